"""Section f15 of include/iivision.h (picture levels) and the two table builders of frame_grabber.py, restated in numpy: what
csrc/iiv_levels.hip and the Python layer must equal byte for byte and count for count.  Nothing here imports the product."""
import numpy as np

LUMA = (77, 150, 29)


def luma(rgb):
    """Y = (77 R + 150 G + 29 B + 128) >> 8 of uint8 (..., 3) -> int64 (...)"""
    a = np.asarray(rgb).astype(np.int64)
    return (LUMA[0] * a[..., 0] + LUMA[1] * a[..., 1] + LUMA[2] * a[..., 2] + 128) >> 8


def histogram(frames):
    """uint8 (..., pixels, 3) -> uint32 (..., 4, 256): per leading index the counts of R, G, B and Y"""
    a = np.asarray(frames)
    lead = a.shape[:-2]
    flat = a.reshape((-1,) + a.shape[-2:])
    out = np.zeros((flat.shape[0], 4, 256), np.uint32)
    for i, f in enumerate(flat):
        for c in range(3):
            out[i, c] = np.bincount(f[:, c], minlength=256)
        out[i, 3] = np.bincount(luma(f), minlength=256)
    return out.reshape(lead + (4, 256))


def auto(hist, lo_ppm=5000, hi_ppm=5000):
    """(black, white) of 256 counts, in Python integers"""
    h = [int(v) for v in hist]
    total = sum(h)
    k_lo, k_hi = total * lo_ppm // 10 ** 6, total * hi_ppm // 10 ** 6
    if total == 0:
        return 0, 255
    cum = lambda v: sum(h[:v + 1])     # noqa: E731  (cum(-1) = 0)
    black = min(v for v in range(256) if cum(v) > k_lo)
    white = max(v for v in range(256) if total - cum(v - 1) > k_hi)
    return (0, 255) if white <= black else (black, white)


def linear_lut(black, white):
    """L[v] = clamp(floor((510 (v - black) + D) / (2 D)), 0, 255), D = white - black, in Python integers"""
    d = white - black
    return np.array([min(max((510 * (v - black) + d) // (2 * d), 0), 255) for v in range(256)], np.uint8)


def curve(gamma, brightness, contrast):
    """C[u], the float64 curve of frame_grabber.levels_lut, rounded half up and clipped"""
    u = np.arange(256, dtype=np.float64) / 255.0
    return np.clip(np.floor(255.0 * ((u ** (1.0 / gamma) - 0.5) * contrast + 0.5) + brightness + 0.5), 0, 255).astype(np.uint8)


def levels_lut(black=0, white=255, gamma=1.0, brightness=0, contrast=1.0):
    lin = linear_lut(black, white)
    if gamma == 1.0 and brightness == 0 and contrast == 1.0:
        return lin
    return curve(gamma, brightness, contrast)[lin]


def saturation_matrix(s256):
    o_r, o_b = ((256 - s256) * LUMA[0] + 128) >> 8, ((256 - s256) * LUMA[2] + 128) >> 8
    o = [o_r, (256 - s256) - o_r - o_b, o_b]
    return np.array([[o[k] + (s256 if c == k else 0) for k in range(3)] for c in range(3)], np.int64)


IDENTITY_LUT = np.arange(256, dtype=np.uint8)
IDENTITY_MATRIX = 256 * np.eye(3, dtype=np.int64)


def apply(frames, lut, matrix=None):
    """uint8 (..., 3) through lut -- (256,) or (3, 256) -- and matrix (3, 3) integers: a_c = lut[c][x_c],
    y_c = clamp((m[c] . a + 128) >> 8, 0, 255) with the arithmetic shift"""
    x = np.asarray(frames)
    lut = np.broadcast_to(np.asarray(lut), (3, 256))
    m = np.asarray(IDENTITY_MATRIX if matrix is None else matrix).astype(np.int64)
    a = np.stack([lut[c][x[..., c]] for c in range(3)], axis=-1).astype(np.int64)
    y = (a @ m.T + 128) >> 8
    return np.clip(y, 0, 255).astype(np.uint8)


def apply_clips(frames, luts, matrices):
    """uint8 (c, ..., 3) with luts (c, 3, 256) and matrices (c, 3, 3)"""
    return np.stack([apply(f, l, m) for f, l, m in zip(frames, luts, matrices)])
