"""The planes that show the 4:2:0 conversion of include/iivision.h f11 every (Y, U, V) triple, 2^24 of them, exactly once; the
sums the contract shifts and clamps, restated so that a test can ask where they leave 0..255; and the matrices the exhaustive
tests run (tests/test_gpu_yuv_exhaustive.py on the device, tests/test_yuv_model.py for the conditions on the model alone).

    B1  same-size frames (yuv_to_rgb_kernel): 16 frames of 1024 x 1024.  The 2 x 2 chroma block b = 0 .. 2^22 - 1, numbered by
        frame, chroma row, chroma column, carries U = b & 255, V = (b >> 8) & 255 and the four luma samples 4 (b >> 16) + 2 dy + dx.
    B2  constant rows (the fused loader of resize_h_kernel<2, YuvRows>): 16384 frames of 1024 rows (the horizontal pass alone needs
        H == h, and H is at most 1024).  Row pair p = 0 .. 2^23 - 1, numbered by frame, chroma row, carries (U, V) = (p & 255,
        (p >> 8) & 255); its rows carry Y = 2 (p >> 16) + dy.  The planes are one column wide here; widen() repeats it.
    B3  constant rows for the one-row form (w > 4096): frames of two rows; half of them hold a triple on the boundary of a clamp
        in their first row and another luma under the same chroma in their second, half of them uniform triples.
"""
import numpy as np

import yuv_model

PRESETS = ("bt601", "bt709", "jpeg")
# at the argument bounds, opposite sign patterns
BOUNDS_MATRICES = ((255, 1023, -1023, 1023, -1023, 1023), (0, 1023, 1023, -1023, -1023, -1023))
# sum >> 8 over all triples and channels under BOUNDS_MATRICES: the extremes of the contract
BOUNDS_EXTREMES = ((-2038, 1019), (-1015, 2042))
# the values of sum >> 8 next to the clamps: the last one clamped to 0, the first and last ones kept, the first one clamped to 255
EDGE_VALUES = (-1, 0, 255, 256)
B1_SHAPE = (16, 1024, 1024)
B2_SHAPE = (16384, 1024)
B3_WIDTH, B3_FRAMES = 4100, 2048


def _readonly(*planes):
    for p in planes:
        p.setflags(write=False)
    return planes


def b1_planes():
    """-> y (16, 1024, 1024), u, v (16, 512, 512)"""
    n, h, w = B1_SHAPE
    b = np.arange(n * (h // 2) * (w // 2), dtype=np.int64).reshape(n, h // 2, w // 2)
    y = np.empty(B1_SHAPE, np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            y[:, dy::2, dx::2] = 4 * (b >> 16) + 2 * dy + dx
    return _readonly(y, (b & 255).astype(np.uint8), ((b >> 8) & 255).astype(np.uint8))


def b2_columns():
    """-> y (16384, 1024, 1), u, v (16384, 512, 1): one column of the constant rows"""
    n, h = B2_SHAPE
    p = np.arange(n * (h // 2), dtype=np.int64).reshape(n, h // 2, 1)
    y = np.empty((n, h, 1), np.uint8)
    for dy in (0, 1):
        y[:, dy::2] = 2 * (p >> 16) + dy
    return _readonly(y, (p & 255).astype(np.uint8), ((p >> 8) & 255).astype(np.uint8))


def widen(y, u, v, w):
    """planes one column wide -> the same rows w pixels wide (contiguous)"""
    cw = (w + 1) // 2
    return (np.ascontiguousarray(np.broadcast_to(y, y.shape[:2] + (w,))), np.ascontiguousarray(np.broadcast_to(u, u.shape[:2] + (cw,))),
            np.ascontiguousarray(np.broadcast_to(v, v.shape[:2] + (cw,))))


def shifted_sums(y, u, v, matrix):
    """(ky c + ... + 128) >> 8 of the contract, before the clamp: int32 (..., 3) for arrays y, u, v of one shape (a triple per
    element: the chroma sample already chosen)"""
    y_off, ky, rv, gu, gv, bu = (int(k) for k in (yuv_model.MATRICES[matrix] if isinstance(matrix, str) else matrix))
    c = ky * (np.asarray(y).astype(np.int32) - y_off) + 128
    d, e = np.asarray(u).astype(np.int32) - 128, np.asarray(v).astype(np.int32) - 128
    return np.stack([c + rv * e, c + gu * d + gv * e, c + bu * d], axis=-1) >> 8


def upsampled(u, h, w):
    """the chroma sample of every pixel of (..., h, w) frames: sample (y >> 1, x >> 1)"""
    return u[..., np.arange(h) >> 1, :][..., np.arange(w) >> 1]


def triple_keys(y, u, v):
    """Y << 16 | U << 8 | V per pixel of (n, h, w) planes with (n, ch, cw) chroma"""
    h, w = y.shape[-2:]
    return (y.astype(np.int64) << 16) | (upsampled(u, h, w).astype(np.int64) << 8) | upsampled(v, h, w).astype(np.int64)


def all_triples():
    """-> y, u, v uint8 (2^24,): every triple, Y slowest"""
    k = np.arange(1 << 24, dtype=np.int32)
    return (k >> 16).astype(np.uint8), ((k >> 8) & 255).astype(np.uint8), (k & 255).astype(np.uint8)


def boundary_triples(matrix):
    """-> (K, 3) uint8: the triples with a channel whose sum >> 8 is one of EDGE_VALUES -- or, under a matrix for which none of
    those exists in a channel, that channel's extremes"""
    y, u, v = all_triples()
    s = shifted_sums(y, u, v, matrix)
    hit = np.zeros(len(y), bool)
    for c in range(3):
        edge = np.isin(s[:, c], EDGE_VALUES)
        hit |= edge if edge.any() else (s[:, c] == s[:, c].min()) | (s[:, c] == s[:, c].max())
    return np.stack([y[hit], u[hit], v[hit]], axis=1)


def b3_columns(matrix, seed=23):
    """-> y (2048, 2, 1), u, v (2048, 1, 1): one column of the constant rows.  Frames 0..1023: row 0 a seeded sample of
    boundary_triples(matrix), row 1 a uniform luma under the same chroma; frames 1024..2047: uniform triples"""
    rng = np.random.RandomState(seed)
    half = B3_FRAMES // 2
    edge = boundary_triples(matrix)
    pick = edge[rng.choice(len(edge), half, replace=len(edge) < half)]
    y = rng.randint(0, 256, (B3_FRAMES, 2, 1)).astype(np.uint8)
    u, v = rng.randint(0, 256, (B3_FRAMES, 1, 1)).astype(np.uint8), rng.randint(0, 256, (B3_FRAMES, 1, 1)).astype(np.uint8)
    y[:half, 0, 0], u[:half, 0, 0], v[:half, 0, 0] = pick[:, 0], pick[:, 1], pick[:, 2]
    return _readonly(y, u, v)
