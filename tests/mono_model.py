"""Mono playback mode, restated in numpy from its contract (include/iivision.h: iiv_frames_to_memory_maps_mono and the
cost matrix beside it).  The yardstick of csrc/iiv_mono.hip and of palette.MonoPalette.diff_matrix(): written from the
contract, not from the kernels.

    dm_mono()                          the 16 x 16 cost matrix
    luma(rgb)                          (..., 3) uint8 -> int Y
    dots(rgb, dither)                  (n, 192, W, 3) uint8 -> (n, 192, W) uint8 of 0 / 1
    pack(mode, dots)                   -> (main, aux) (n, 32, 256) uint8 memory maps (aux None for HGR)
    frames_to_memory_maps(mode, rgb, dither)   the two together
Error diffusion comes twice: diffuse_raster is the definition as it is written (a Python loop over every dot, in raster
order); diffuse is the same sums taken along the anti-diagonals x + 2 y = t (every dot on one depends only on earlier
ones), whole diagonals at a time -- tests/test_mono_host.py holds the two equal.
"""
import numpy as np

HGR, DHGR = 0, 1
DITHER_DIFFUSION = 256
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], dtype=np.int64)


def width(mode):
    return 560 if mode == DHGR else 280


def popcount4(v):
    return (v & 1) + ((v >> 1) & 1) + ((v >> 2) & 1) + ((v >> 3) & 1)


def dm_mono():
    a = np.arange(16)[:, None]
    b = np.arange(16)[None, :]
    return (16 * np.abs(popcount4(a) - popcount4(b)) + 8 * popcount4(a ^ b)).astype(np.int32)


def y_to_offset(y):
    """y_to_base_addr(y, 0) - 0x2000 (screen.py:16-22)"""
    a, d = divmod(y, 64)
    b, c = divmod(d, 8)
    return 1024 * c + 128 * b + 40 * a


def luma(rgb):
    rgb = np.asarray(rgb).astype(np.int64)
    return (77 * rgb[..., 0] + 150 * rgb[..., 1] + 29 * rgb[..., 2] + 128) >> 8


def ordered(Y, dither):
    """Y: (n, 192, W) int -> dots"""
    H, W = Y.shape[1:]
    off = np.floor_divide((2 * BAYER - 15) * int(dither), 16)            # floor, towards minus infinity
    d = off[np.arange(H)[:, None] & 3, np.arange(W)[None, :] & 3]
    v = np.clip(Y + d[None], 0, 255)
    return (v >= 128).astype(np.uint8)


def diffuse_raster(Y):
    """Floyd-Steinberg exactly as the contract words it.  Y: (n, H, W) int -> dots.  Slow: a Python loop over H x W."""
    n, H, W = Y.shape
    acc = np.zeros((n, H + 1, W + 2), dtype=np.int64)                    # a border takes what falls outside
    out = np.zeros((n, H, W), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            v = np.clip(Y[:, y, x] + (acc[:, y, x + 1] >> 4), 0, 255)    # >> of a negative int64 is a floor
            dot = v >= 128
            e = v - 255 * dot
            out[:, y, x] = dot
            acc[:, y, x + 2] += 7 * e
            acc[:, y + 1, x] += 3 * e
            acc[:, y + 1, x + 1] += 5 * e
            acc[:, y + 1, x + 2] += e
        acc[:, y + 1, 0] = 0
        acc[:, y + 1, W + 1] = 0
    return out


def diffuse(Y):
    """The same function, a whole anti-diagonal x + 2 y = t per step: dot (x, y) takes from (x - 1, y), (x - 1, y - 1),
    (x, y - 1), (x + 1, y - 1), which lie on the diagonals t - 1, t - 3, t - 2, t - 1."""
    n, H, W = Y.shape
    E = np.zeros((n, H + 1, W + 2), dtype=np.int64)                      # e of (y, x) at [y + 1, x + 1]; zero outside
    out = np.zeros((n, H, W), dtype=np.uint8)
    for t in range(W + 2 * (H - 1)):
        ys = np.arange(max(0, (t - W + 2) // 2), min(H - 1, t // 2) + 1)
        xs = t - 2 * ys
        acc = 7 * E[:, ys + 1, xs] + E[:, ys, xs] + 5 * E[:, ys, xs + 1] + 3 * E[:, ys, xs + 2]
        v = np.clip(Y[:, ys, xs] + (acc >> 4), 0, 255)
        dot = v >= 128
        out[:, ys, xs] = dot
        E[:, ys + 1, xs + 1] = v - 255 * dot
    return out


def dots(rgb, dither, raster=False):
    Y = luma(rgb)
    if int(dither) == DITHER_DIFFUSION:
        return diffuse_raster(Y) if raster else diffuse(Y)
    if not 0 <= int(dither) <= 255:
        raise ValueError("dither")
    return ordered(Y, dither)


def pack(mode, d):
    """dots (n, 192, W) -> memory maps: dot X = bit X % 7 of byte X / 7 of the row; DHGR: even bytes aux, odd bytes main,
    column X / 14; HGR: all 40 bytes main; bit 7 clear; holes 0."""
    d = np.asarray(d)
    n, H, W = d.shape
    assert H == 192 and W == width(mode)
    rowbytes = (d.reshape(n, H, W // 7, 7).astype(np.uint16) << np.arange(7, dtype=np.uint16)).sum(axis=3).astype(np.uint8)
    main = np.zeros((n, 8192), dtype=np.uint8)
    aux = np.zeros((n, 8192), dtype=np.uint8) if mode == DHGR else None
    for y in range(192):
        o = y_to_offset(y)
        if mode == DHGR:
            aux[:, o:o + 40] = rowbytes[:, y, 0::2]
            main[:, o:o + 40] = rowbytes[:, y, 1::2]
        else:
            main[:, o:o + 40] = rowbytes[:, y]
    return main.reshape(n, 32, 256), (aux.reshape(n, 32, 256) if aux is not None else None)


def frames_to_memory_maps(mode, rgb, dither=0):
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.shape[1:] == (192, width(mode), 3)
    return pack(mode, dots(rgb, dither))


def unpack(mode, main, aux=None):
    """The inverse of pack for one frame: (192, W) dots, read straight from the bytes."""
    W = width(mode)
    out = np.zeros((192, W), dtype=np.uint8)
    m = np.asarray(main).reshape(8192)
    a = np.asarray(aux).reshape(8192) if aux is not None else None
    for y in range(192):
        o = y_to_offset(y)
        if mode == DHGR:
            row = np.empty(80, dtype=np.uint8)
            row[0::2] = a[o:o + 40]
            row[1::2] = m[o:o + 40]
        else:
            row = m[o:o + 40]
        out[y] = ((row[:, None] >> np.arange(7)) & 1).reshape(W)
    return out


# ---- the inputs the tests share ------------------------------------------------------------

def structured_frames(mode, n, seed=0):
    """picture-like frames: colour bars drifting over ramps, a disc, some noise"""
    W = width(mode)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:192, 0:W]
    bars = np.array([[255, 255, 255], [255, 255, 0], [0, 255, 255], [0, 255, 0], [255, 0, 255], [255, 0, 0], [0, 0, 255], [0, 0, 0]], np.uint8)
    out = np.empty((n, 192, W, 3), np.uint8)
    for f in range(n):
        out[f] = bars[((x + 5 * f) // (W // 8)) % 8]
        out[f, 96:] = ((x[96:] * 256 // W + y[96:] - 3 * f) % 256)[..., None]
        disc = (x - W // 2 - 7 * f) ** 2 // (4 if mode == DHGR else 1) + (y - 96) ** 2 < 50 ** 2
        out[f][disc] = (out[f][disc].astype(np.int64) * 3 // 4 + rng.integers(0, 64, (int(disc.sum()), 3))).astype(np.uint8)
    return out


def corner_frames(mode):
    """black, white, the saturated primaries, a one-dot checkerboard, steep ramps both ways, a vertical ramp"""
    W = width(mode)
    y, x = np.mgrid[0:192, 0:W]
    fr = []
    for c in ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)):
        fr.append(np.broadcast_to(np.array(c, np.uint8), (192, W, 3)).copy())
    fr.append(np.broadcast_to((((x + y) & 1) * 255).astype(np.uint8)[..., None], (192, W, 3)).copy())
    steep = np.clip((x % 32) * 64 - 512, 0, 255)          # 0 .. 255 in four dots, over and over: the accumulators hit the clamps
    fr.append(np.broadcast_to(steep.astype(np.uint8)[..., None], (192, W, 3)).copy())
    fr.append(np.broadcast_to((255 - steep).astype(np.uint8)[..., None], (192, W, 3)).copy())
    fr.append(np.broadcast_to(np.clip((y % 24) * 80 - 400, 0, 255).astype(np.uint8)[..., None], (192, W, 3)).copy())
    return np.stack(fr)


def noise_frames(mode, n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, 192, width(mode), 3), dtype=np.uint8)
