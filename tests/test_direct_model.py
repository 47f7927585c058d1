"""CPU: tests/direct_model.py -- the numpy restatement of "f10: direct ingest" (include/iivision.h) -- held to the contract's
GLOBAL rule from outside: everything a row costs here is measured through tests/render_model.py's dot and colour rules.
  brute force          2-byte rows in both modes and 3-byte DHGR rows (2^21 candidates): the model's row is the exhaustive
                       minimum under the tie rule, on random targets and on flat ones, which tie heavily
  second formulation   full rows: a byte-level dynamic program, eight states (the top three bits of the byte to the left), whose
                       inner step tries every byte value literally, gives the same bytes and cost
  perturbations        full rows: no single-byte replacement costs less; at equal cost the replacement is the larger byte
  screen error         dither 0: the frame cost is render_error_model's level 0 summed over the channels, at both widths
  other converters     the frame cost is <= that sum for the maps of ingest_model (ordered, diffusion) and diffusion_model
  layout               holes 0, DHGR bit 7 clear
  HGR shift cases      rows whose best first / last byte has its palette bit set (the last one: the dropped 561st dot)"""
import numpy as np
import pytest

import diffusion_model
import direct_model as D
import ingest_model
import render_error_model as E
import render_model as R

MODES = [R.HGR, R.DHGR]
DISTINCT = ((np.arange(48) * 37 + 11) % 256).astype(np.uint8).reshape(16, 3)
PAIRS = ingest_model.PALETTES["pairs"]              # value c and c ^ 8 alike: ties between different rows


def _ntsc():
    import palette
    return np.asarray(palette.NTSCPalette.rgb_array(), dtype=np.uint8).reshape(16, 3)


def values_of_rows(mode, rows):
    """(M, L) byte rows, each the beginning of a screen row of zeros -> (M, dots of L bytes) colour values by render_model"""
    rows = np.asarray(rows, dtype=np.uint8)
    M, L = rows.shape
    n_maps = -(-M // 192)
    full = np.zeros((n_maps * 192, D.ROW_BYTES[mode]), np.uint8)
    full[:M, :L] = rows
    main, aux = D.place(mode, full.reshape(n_maps, 192, -1))
    return R.colour_values(mode, main, aux).reshape(n_maps * 192, R.WIDTH)[:M, :D.DOTS_PER_BYTE[mode] * L]


def cost_of_values(pal, values, T):
    """values (M, X), T (X, 3) -> (M,) int64"""
    d = np.asarray(pal, dtype=np.int64).reshape(16, 1, 3) - np.asarray(T, dtype=np.int64)[None]
    per_dot = (d * d).sum(axis=2)                                    # [colour value][x]
    return per_dot[values, np.arange(values.shape[1])[None, :]].sum(axis=1)


def cost_of_rows(mode, pal, rows, T):
    return cost_of_values(pal, values_of_rows(mode, rows), T)


_CANDIDATES = {}


def candidate_values(mode, L):
    """every legal row of L <= 3 bytes in the order of its number -> its colour values, computed once.  Candidates lie four
    bytes apart in the screen rows handed to render_model, zero bytes between them: four bytes are 28 or 56 dots, a multiple
    of four, so each sees the phases, the three dots of 0 to its left and (HGR) the bit 6 of 0 that a row's beginning sees."""
    if (mode, L) not in _CANDIDATES:
        base, nb, dots = (128, 80, 7 * L) if mode == R.DHGR else (256, 40, 14 * L)
        per_row, stride = nb // 4, R.WIDTH * 4 // nb
        j = np.arange(base ** L)
        cand = np.zeros((-(-len(j) // per_row) * per_row, 4), np.uint8)
        for i in range(L):
            cand[:len(j), i] = (j // base ** i) % base
        v = values_of_rows(mode, cand.reshape(-1, nb)).reshape(-1, per_row, stride)
        _CANDIDATES[mode, L] = v[:, :, :dots].reshape(-1, dots)[:len(j)]
    return _CANDIDATES[mode, L]


def _targets(X, seed):
    rng = np.random.default_rng(seed)
    flat = [np.broadcast_to(np.array(c), (X, 3)) for c in ((0, 0, 0), (255, 255, 255), (128, 128, 128), (90, 75, 5), (201, 30, 88))]
    return [rng.integers(0, 256, (X, 3)) for _ in range(4)] + flat + [np.repeat(rng.integers(0, 256, (X // 7, 3)), 7, axis=0)]


@pytest.mark.parametrize("mode,L", [(R.HGR, 2), (R.DHGR, 2), (R.DHGR, 3)])
def test_short_rows_are_the_exhaustive_minimum(mode, L):
    base = 128 if mode == R.DHGR else 256
    values = candidate_values(mode, L)
    assert values.shape == (base ** L, D.DOTS_PER_BYTE[mode] * L)
    for pal in (DISTINCT, PAIRS, _ntsc(), ingest_model.PALETTES["all_equal"]):
        for t, T in enumerate(_targets(values.shape[1], 5 + L)[::3 if L == 3 else 1]):
            cost = cost_of_values(pal, values, T)
            j = int(cost.argmin())                                   # the first minimum: the smallest number
            want = [(j // base ** i) % base for i in range(L)]
            row, got = D.best_rows(mode, pal, T, L)
            assert got == cost[j] and row.tolist() == want, (t, row.tolist(), want, int(got), int(cost[j]))


# ---- the second formulation: bytes, not dots

_BYTE_VALUES = {}


def byte_values(mode):
    """[i][t][v] -> the colour values of the dots of byte i with value v behind a byte whose top three bits (DHGR: bits 6..4,
    HGR: 7..5) are t, through render_model: (row bytes, 8, 128 or 256, 7 or 14)"""
    if mode not in _BYTE_VALUES:
        nb, dpb, top = D.ROW_BYTES[mode], D.DOTS_PER_BYTE[mode], 4 if mode == R.DHGR else 5
        nv = 128 if mode == R.DHGR else 256
        rows = np.zeros((nb, 8, nv, nb), np.uint8)
        for i in range(nb):
            rows[i, :, :, i] = np.arange(nv)[None, :]
            if i:
                rows[i, :, :, i - 1] = (np.arange(8) << top)[:, None]
        v = values_of_rows(mode, rows.reshape(-1, nb)).reshape(nb, 8, nv, R.WIDTH)
        _BYTE_VALUES[mode] = np.stack([v[i, :, :, dpb * i:dpb * (i + 1)] for i in range(nb)])
    return _BYTE_VALUES[mode]


def best_row_by_bytes(mode, pal, T):
    nb, dpb, top = D.ROW_BYTES[mode], D.DOTS_PER_BYTE[mode], 4 if mode == R.DHGR else 5
    pal = np.asarray(pal, dtype=np.int64).reshape(16, 3)
    V = byte_values(mode)
    nv = V.shape[2]
    d = pal[V] - np.asarray(T, dtype=np.int64).reshape(nb, 1, 1, dpb, 3)
    cost = (d * d).sum(axis=(3, 4))                                  # [i][t of the byte to the left][v]
    big = 1 << 40
    Ev = [np.array([0] + [big] * 7)]                                  # nothing left of the row: dots of 0
    for i in range(nb):
        through = Ev[-1][:, None] + cost[i]                           # [t left][v]
        Ev.append(np.array([through[:, (np.arange(nv) >> top) == t].min() for t in range(8)]))
    t = int(Ev[-1].argmin())
    total, row = int(Ev[-1][t]), []
    for i in range(nb - 1, -1, -1):
        found = None
        for v in range(t << top, (t + 1) << top):                     # the byte's own bits before the byte to the left
            for left in range(8):
                if Ev[i][left] + cost[i][left][v] == Ev[i + 1][t]:
                    found = (v, left)
                    break
            if found:
                break
        row.append(found[0])
        t = found[1]
    return row[::-1], total


def _rows_under_test(mode):
    """a few targets of full rows: noise, picture-like runs, flat ones"""
    rng = np.random.default_rng(40 + mode)
    smooth = np.repeat(rng.integers(0, 256, (80, 3)), 7, axis=0)
    card = np.stack([np.arange(560) * 255 // 559, np.arange(560)[::-1] * 255 // 559, (np.arange(560) * 3) % 256], axis=1)
    return [rng.integers(0, 256, (560, 3)), smooth, card, np.full((560, 3), 128), np.zeros((560, 3), np.int64), np.full((560, 3), 255)]


@pytest.mark.parametrize("mode", MODES)
def test_full_rows_equal_the_byte_level_program(mode):
    for pal in (_ntsc(), PAIRS):
        for k, T in enumerate(_rows_under_test(mode)):
            row, cost = D.best_rows(mode, pal, T)
            want, total = best_row_by_bytes(mode, pal, T)
            assert int(cost) == total and row.tolist() == want, (k, int(cost), total)


@pytest.mark.parametrize("mode", MODES)
def test_no_single_byte_replacement_is_better(mode):
    nb = D.ROW_BYTES[mode]
    nv = 128 if mode == R.DHGR else 256
    for pal in (_ntsc(), PAIRS):
        for k, T in enumerate(_rows_under_test(mode)[:4]):
            row, cost = D.best_rows(mode, pal, T)
            assert cost_of_rows(mode, pal, row[None], T)[0] == cost
            variants = np.broadcast_to(row, (nb, nv, nb)).copy()
            variants[np.arange(nb), :, np.arange(nb)] = np.arange(nv)[None, :]
            c = cost_of_rows(mode, pal, variants.reshape(-1, nb), T).reshape(nb, nv)
            assert (c >= cost).all(), k
            smaller = np.arange(nv)[None, :] < row[:, None]
            assert not ((c == cost) & smaller).any(), k              # (equal cost and a smaller byte: a smaller number)


def _frames(width, seed):
    """(3, 192, width, 3): noise, picture-like blocks, a gradient"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:192, 0:width]
    blocks = rng.integers(0, 256, (24, 35, 3)).repeat(8, axis=0).repeat(width // 35, axis=1)
    grad = np.stack([x * 255 // (width - 1), y * 255 // 191, (x + y) * 255 // (width + 190)], axis=-1)
    return np.stack([rng.integers(0, 256, (192, width, 3)), blocks, grad]).astype(np.uint8)


@pytest.fixture(scope="module")
def converted():
    """(mode, width) -> (frames, palette, main, aux, cost) at dither 0, computed once"""
    out = {}
    for mode in MODES:
        for width in (280, 560):
            rgb, pal = _frames(width, 7 * width + mode), _ntsc()
            out[mode, width] = (rgb, pal) + D.frames_to_memory_maps_direct(mode, pal, rgb, 0)
    return out


def _level0(mode, pal, main, aux, rgb):
    return E.render_error(mode, main, aux, pal, rgb)[:, 0, :].sum(axis=1)


@pytest.mark.parametrize("width", [280, 560])
@pytest.mark.parametrize("mode", MODES)
def test_frame_cost_is_the_screen_error(converted, mode, width):
    rgb, pal, main, aux, cost = converted[mode, width]
    assert cost.dtype == np.uint64 and (cost == _level0(mode, pal, main, aux, rgb)).all()


@pytest.mark.parametrize("mode", MODES)
def test_never_worse_than_the_other_converters(converted, mode):
    rgb, pal, _, _, cost = converted[mode, 280]
    others = {"ordered 0": ingest_model.frames_to_memory_maps(mode, pal, rgb, 0),
              "ordered 32": ingest_model.frames_to_memory_maps(mode, pal, rgb, 32),
              "diffusion": ingest_model.frames_to_memory_maps(mode, pal, rgb, ingest_model.DITHER_DIFFUSION)}
    for name in ("atkinson", "jarvis"):
        w, divisor = diffusion_model.KERNELS[name]
        others[name] = diffusion_model.frames_to_memory_maps(mode, pal, rgb, w, divisor)
    for name, (main, aux) in others.items():
        assert (cost <= _level0(mode, pal, main, aux, rgb)).all(), name


@pytest.mark.parametrize("mode", MODES)
def test_holes_and_reserved_bits(converted, mode):
    for width in (280, 560):
        _, _, main, aux, _ = converted[mode, width]
        for bank in (main, aux) if mode == R.DHGR else (main,):
            assert bank.shape == (3, 32, 256) and bank.dtype == np.uint8
            assert not bank[:, :, 120:128].any() and not bank[:, :, 248:256].any()
            assert mode == R.HGR or not (bank & 0x80).any()
        assert aux is not None or mode == R.HGR
    assert (converted[R.HGR, 280][2] & 0x80).any()                    # (HGR does use its palette bit)


@pytest.mark.parametrize("pattern", [(0xD5, 0xAA), (0xAA, 0xD5)])
def test_hgr_rows_that_need_the_shift_at_either_end(pattern):
    """A screen row of one shifted colour, rendered, is a target some row meets exactly; with sixteen different colours only
    the same dots do, and their lit pairs start at odd dots: the first and the last byte need their palette bit -- the last
    one (0xD5: bit 6 set) with its 561st dot dropped."""
    row = np.array(pattern * 20, np.uint8)
    main, _ = D.place(R.HGR, np.broadcast_to(row, (1, 192, 40)))
    T = R.render_rgb(R.HGR, main, None, DISTINCT)[0, 0]
    got, cost = D.best_rows(R.HGR, DISTINCT, T)
    assert cost == 0 and got[0] & 0x80 and got[-1] & 0x80, got.tolist()
    assert (values_of_rows(R.HGR, got[None]) == values_of_rows(R.HGR, row[None])).all()
