"""The tests' model of the 4:2:0 YCbCr -> RGB conversion in front of the resize, written in numpy from the contract in
include/iivision.h (f11: iiv_resize_frames_yuv420), not from the kernel.  For source pixel (x, y) of an h x w frame:

    Yv = Y[y][x];  U = Cb[y >> 1][x >> 1];  V = Cr[y >> 1][x >> 1]        the nearest chroma sample, no interpolation
    c = Yv - y_off,  d = U - 128,  e = V - 128
    R = clamp((ky c        + rv e + 128) >> 8, 0, 255)
    G = clamp((ky c + gu d + gv e + 128) >> 8, 0, 255)
    B = clamp((ky c + bu d        + 128) >> 8, 0, 255)                      >> arithmetic (numpy's on signed integers is)

matrix = (y_off, ky, rv, gu, gv, bu).  The RGB frames then go through resize_model.resize unchanged.
"""
import numpy as np

# the presets as the issue and the header state them (frame_grabber.YUV_MATRICES is held to this copy by test_yuv_model.py)
MATRICES = {
    "bt601": (16, 298, 409, -100, -208, 516),
    "bt709": (16, 298, 459, -55, -136, 541),
    "jpeg": (0, 256, 359, -88, -183, 454),
}


def to_rgb(y, u, v, matrix="bt601"):
    """y uint8 (n, h, w) or (h, w); u, v uint8 (..., (h + 1) // 2, (w + 1) // 2) -> uint8 (..., h, w, 3)"""
    y_off, ky, rv, gu, gv, bu = (int(k) for k in (MATRICES[matrix] if isinstance(matrix, str) else matrix))
    y, u, v = (np.asarray(p, np.uint8) for p in (y, u, v))
    h, w = y.shape[-2:]
    assert u.shape == v.shape == y.shape[:-2] + ((h + 1) // 2, (w + 1) // 2), (y.shape, u.shape, v.shape)
    rows, cols = np.arange(h) >> 1, np.arange(w) >> 1
    c = y.astype(np.int64) - y_off
    d = u.astype(np.int64)[..., rows, :][..., cols] - 128
    e = v.astype(np.int64)[..., rows, :][..., cols] - 128
    rgb = np.stack([ky * c + rv * e + 128, ky * c + gu * d + gv * e + 128, ky * c + bu * d + 128], axis=-1) >> 8
    return np.clip(rgb, 0, 255).astype(np.uint8)


def random_planes(n, h, w, seed):
    """seeded random planes (y, u, v) of n frames"""
    rng = np.random.RandomState(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return (rng.randint(0, 256, (n, h, w)).astype(np.uint8), rng.randint(0, 256, (n, ch, cw)).astype(np.uint8),
            rng.randint(0, 256, (n, ch, cw)).astype(np.uint8))
