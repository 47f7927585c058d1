"""numpy restatement of iiv_frames_to_memory_maps_direct's contract (include/iivision.h, "f10: direct ingest"): per screen row
the byte row whose RENDERED dots (f7) are nearest the dithered source, ties to the smallest row read as a number whose last
byte is most significant.  Written from the contract's words, int64 throughout; it takes nothing from the kernel or the
library.  The colour of a window is render_model's (ROL4), the widening of the source render_error_model's, the Bayer matrix
ingest_model's; tests/test_direct_model.py holds the rows found here to render_model's dot rules by exhaustive search.

A row of n_bytes bytes (DHGR: of the aux / main sequence, seven dots each; HGR: fourteen dots each) is found by a forward pass
over the dots and a backtrace.  The state is the last three dots a | b << 1 | c << 2 (c the newest); a step appends one dot and
drops the oldest.  The backtrace fixes choices in descending significance and takes 0 whenever a least-cost completion exists.
  DHGR  dot 7 i + j is bit j of byte i, so later dots are more significant: start from the least-cost end state (ties to the
        smaller state: its newest dot is the most significant), at every step prefer a dropped dot of 0.
  HGR   the state also holds the byte's palette bit p (more significant than the byte's data bits, so chosen at the end of the
        byte) and a dot is either a new data bit or a copy of the dot before it (p = 0: odd dots of the byte's fourteen; p = 1:
        even ones, dot 0 copying the last dot of the byte to the left).  The first four dots of a byte look at dots of the byte to
        the left, whose palette bit p' is MORE significant than its data bits: p' stays in the state over those four dots and
        the two branches meet behind them, ties to p' = 0, so the backtrace meets p' before bit 6 and bit 5 of that byte."""
import numpy as np

import render_error_model as E
import render_model as R
from ingest_model import BAYER

HGR, DHGR = R.HGR, R.DHGR
INF = np.int64(1) << 40
DOTS_PER_BYTE = {HGR: 14, DHGR: 7}
ROW_BYTES = {HGR: 40, DHGR: 80}


def target(rgb, dither):
    """(n, 192, 280 or 560, 3) u8 -> T (n, 192, 560, 3) int64: the source at dot width plus the ordered-dither offset of the
    dot's quad, clamped"""
    assert 0 <= dither <= 255
    y, x = np.arange(R.HEIGHT)[:, None], np.arange(R.WIDTH)[None, :]
    offset = ((2 * BAYER[y & 3, (x >> 2) & 3] - 15) * dither) // 16          # floor towards minus infinity
    return np.clip(E.widen(rgb).astype(np.int64) + offset[:, :, None], 0, 255)


def window_costs(palette_rgb, T):
    """T (..., X, 3) -> (..., X, 16) int64: [x][w] = sum over c of (palette[rol4(w, (x + 1) & 3)][c] - T[x][c])^2, w the window
    d[x - 3] | d[x - 2] << 1 | d[x - 1] << 2 | d[x] << 3"""
    pal = np.asarray(palette_rgb, dtype=np.int64).reshape(16, 3)
    X = T.shape[-2]
    value = R.ROL4[np.arange(16)[None, :], ((np.arange(X) + 1) & 3)[:, None]]      # (X, 16)
    d = pal[value] - np.asarray(T, dtype=np.int64)[..., :, None, :]
    return (d * d).sum(axis=-1)


_S = np.arange(8)
_W0, _W1 = _S << 1, (_S << 1) | 1            # the window of new state s with a dropped dot of 0 / 1; the old state is w & 7


def _step(F, c, new_is_copy):
    """F (..., 8) by state, c (N, 16) by window -> (F', dropped dot (..., 8) uint8).  F may carry axes between N and the state"""
    c = c.reshape((c.shape[0],) + (1,) * (F.ndim - 2) + (16,))
    v0, v1 = F[..., _W0 & 7] + c[..., _W0], F[..., _W1 & 7] + c[..., _W1]
    one = v1 < v0
    Fn = np.where(one, v1, v0)
    if new_is_copy is not None:                        # (..., ) bool over the axes between N and the state: b == c is required
        same = ((_S >> 1) & 1) == ((_S >> 2) & 1)
        Fn = np.where(new_is_copy[..., None] & ~same, INF, Fn)
    return np.minimum(Fn, INF), one.astype(np.uint8)


def _best_dhgr(C, n_bytes):
    N, X = C.shape[0], 7 * n_bytes
    F = np.full((N, 8), INF)
    F[:, 0] = 0
    dropped = []
    for x in range(X):
        F, one = _step(F, C[:, x], None)
        dropped.append(one)
    s = F.argmin(axis=1)                               # (the first of several minima: the smaller state)
    cost = F[np.arange(N), s]
    dots = np.zeros((N, X), np.uint8)
    for x in range(X - 1, -1, -1):
        dots[:, x] = s >> 2
        s = ((s << 1) | dropped[x][np.arange(N), s]) & 7
    row = (dots.reshape(N, n_bytes, 7) << np.arange(7)).sum(axis=2).astype(np.uint8)
    return row, cost


def _best_hgr(C, n_bytes):
    N = C.shape[0]
    n = np.arange(N)
    # F[N][p of this byte][p' of the byte to the left][state]; behind a byte's fourth dot only p' = 0 is in use
    F = np.full((N, 2, 2, 8), INF)
    F[:, :, 0, 0] = 0                                  # nothing left of the row: dots of 0 (p' = 0 stands for "no byte")
    dropped, met = [], []
    r_of = np.arange(14)
    copy = np.stack([(r_of & 1) == 1, (r_of & 1) == 0])          # [p][r]: dot r of the byte repeats the dot before it
    for i in range(n_bytes):
        for r in range(14):
            F, one = _step(F, C[:, 14 * i + r], np.broadcast_to(copy[:, r][:, None], (2, 2)))
            dropped.append(one)
            if r == 3:                                 # the branches of p' meet
                q = F[:, :, 1] < F[:, :, 0]
                met.append(q.astype(np.uint8))
                F = np.stack([np.where(q, F[:, :, 1], F[:, :, 0]), np.full((N, 2, 8), INF)], axis=2)
        G = F[:, :, 0]                                 # (N, p, 8) at the end of byte i -> p' of the next byte
        F = np.broadcast_to(G[:, None], (N, 2, 2, 8)).copy()
    flat = G.reshape(N, 16).argmin(axis=1)             # the smaller p, then the smaller state
    cost = G.reshape(N, 16)[n, flat]
    p, s = flat >> 3, flat & 7
    dots = np.zeros((N, 14 * n_bytes), np.uint8)
    pbit = np.zeros((N, n_bytes), np.uint8)
    for i in range(n_bytes - 1, -1, -1):
        pbit[:, i] = p
        left = np.zeros(N, np.int64)
        for r in range(13, -1, -1):
            if r == 3:
                left = met[i][n, p, s].astype(np.int64)
            x = 14 * i + r
            dots[:, x] = s >> 2
            s = ((s << 1) | dropped[x][n, p, left, s]) & 7
        p = left
    d = dots.reshape(N, n_bytes, 14)
    k = np.arange(7)
    plain, shifted = d[:, :, 2 * k], d[:, :, np.minimum(2 * k + 1, 13)]
    data = np.where(pbit[:, :, None] == 1, shifted, plain)
    row = ((data.astype(np.int64) << k).sum(axis=2) | (pbit.astype(np.int64) << 7)).astype(np.uint8)
    return row, cost


def best_rows(mode, palette_rgb, T, n_bytes=None):
    """T (..., X, 3), X = 7 n_bytes (DHGR) or 14 n_bytes (HGR) dots of target -> (rows (..., n_bytes) u8, costs (...) int64).
    n_bytes defaults to a whole row's (80 / 40); a short row is the beginning of a screen row."""
    T = np.asarray(T, dtype=np.int64)
    n_bytes = ROW_BYTES[mode] if n_bytes is None else n_bytes
    assert T.shape[-2] == DOTS_PER_BYTE[mode] * n_bytes and T.shape[-1] == 3
    lead = T.shape[:-2]
    C = window_costs(palette_rgb, T.reshape((-1,) + T.shape[-2:]))
    row, cost = (_best_dhgr if mode == DHGR else _best_hgr)(C, n_bytes)
    return row.reshape(lead + (n_bytes,)), cost.reshape(lead)


def number(rows):
    """(..., L) bytes -> python ints (object array): sum b[i] * 256^i"""
    rows = np.asarray(rows, dtype=np.uint8)
    flat = rows.reshape(-1, rows.shape[-1])
    return np.array([int.from_bytes(r.tobytes(), "little") for r in flat], dtype=object).reshape(rows.shape[:-1])


def place(mode, rows):
    """(n, 192, 80 or 40) byte rows -> (main, aux) (n, 32, 256) u8 memory maps, holes 0; aux is None for HGR"""
    n = rows.shape[0]
    at = R.ROW_OFFSET[:, None] + np.arange(40)[None, :]
    main = np.zeros((n, 8192), np.uint8)
    if mode == HGR:
        main[:, at] = rows
        return main.reshape(n, 32, 256), None
    aux = np.zeros((n, 8192), np.uint8)
    aux[:, at], main[:, at] = rows[:, :, 0::2], rows[:, :, 1::2]
    return main.reshape(n, 32, 256), aux.reshape(n, 32, 256)


def frames_to_memory_maps_direct(mode, palette_rgb, rgb, dither=0):
    """rgb (n, 192, 280 or 560, 3) u8 -> (main, aux, cost): (n, 32, 256) u8 maps (aux None for HGR), (n,) uint64 frame costs"""
    rgb = np.asarray(rgb, dtype=np.uint8)
    rows, cost = best_rows(mode, palette_rgb, target(rgb, dither))
    main, aux = place(mode, rows)
    return main, aux, cost.sum(axis=1).astype(np.uint64)
