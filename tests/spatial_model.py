"""Section f16 of include/iivision.h -- the spatial filter -- restated in numpy, integers only: the blur as the direct 25-term sum
over the clamped 5 x 5 neighbourhood (not the separable form the kernel uses, so model and kernel share no shortcut), then the gain
on the difference.  blur_separable is the header's h / B form, held equal to the direct sum in tests/test_spatial_model.py."""
import numpy as np


def _shifted(p, axis, k, size):
    """p with index i along `axis` holding p[clamp(i + k, 0, size - 1)]"""
    return np.take(p, np.clip(np.arange(size) + k, 0, size - 1), axis=axis)


def blur(frames, taps_x, taps_y):
    """uint8 (..., H, W, 3) -> int64 of the same shape: B = (sum_j sum_k taps_y[j] taps_x[k] p(x + k - 2, y + j - 2) + 32768) >> 16"""
    p = np.asarray(frames).astype(np.int64)
    H, W = p.shape[-3], p.shape[-2]
    acc = np.zeros(p.shape, np.int64)
    for j in range(5):
        rows = _shifted(p, p.ndim - 3, j - 2, H)
        for k in range(5):
            if taps_y[j] and taps_x[k]:
                acc += int(taps_y[j]) * int(taps_x[k]) * _shifted(rows, p.ndim - 2, k - 2, W)
    return (acc + 32768) >> 16


def blur_separable(frames, taps_x, taps_y):
    """the header's two steps: h (0..65280) along x, then B along y"""
    p = np.asarray(frames).astype(np.int64)
    H, W = p.shape[-3], p.shape[-2]
    h = sum(int(taps_x[k]) * _shifted(p, p.ndim - 2, k - 2, W) for k in range(5))
    assert h.min() >= 0 and h.max() <= 65280
    return (sum(int(taps_y[j]) * _shifted(h, p.ndim - 3, j - 2, H) for j in range(5)) + 32768) >> 16


def blend(frames, B, gain):
    """d = p - B, m = max over the channels of |d|, y = clamp(p + ((gain[m] d + 128) >> 8), 0, 255) -> uint8"""
    p = np.asarray(frames).astype(np.int64)
    g = np.asarray(gain).astype(np.int64)
    assert g.shape == (256,)
    d = p - B
    m = np.abs(d).max(axis=-1)
    return np.clip(p + ((g[m][..., None] * d + 128) >> 8), 0, 255).astype(np.uint8)


def check_tables(taps_x, taps_y, gain):
    for t in (taps_x, taps_y):
        t = [int(v) for v in t]
        assert len(t) == 5 and min(t) >= 0 and max(t) <= 256 and sum(t) == 256, t
    g = np.asarray(gain)
    assert g.shape == (256,) and int(g.min()) >= -256 and int(g.max()) <= 1024


def filter_frames(frames, taps_x, taps_y, gain):
    """uint8 (..., H, W, 3) -> uint8 of the same shape"""
    check_tables(taps_x, taps_y, gain)
    return blend(frames, blur(frames, taps_x, taps_y), gain)
