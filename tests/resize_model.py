"""The tests' model of the reference's per-frame resize (frame_grabber.py:75,100:
`_frame.resize((280, 192), resample=Image.LANCZOS)`), written in numpy from the contract in include/iivision.h
(iiv_resize_coeffs / iiv_resize_frames) and DESIGN.md 11:

    coefficients   float64 Lanczos-3 weights per output sample, normalised, rounded to 22-bit fixed point
    one pass       clamp((2^21 + sum(pixel * k)) >> 22, 0, 255) in int32, each channel on its own
    passes         the horizontal pass first (vertical first when h > 100 w); the first pass's uint8 result feeds the
                   second; an axis whose size does not change gets no pass
"""
import math

import numpy as np

PRECISION_BITS = 22
SUPPORT = 3.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3.0)
    return 0.0


def coeffs(in_size, out_size):
    """-> (ksize, bounds int32 (out, 2) = (xmin, count), fixed-point int32 (out, ksize), zero past count)"""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, k


def _pass(a, axis, out_size):
    """one pass of uint8 (n, h, w, 3) along axis 1 (vertical) or 2 (horizontal)"""
    in_size = a.shape[axis]
    _, bounds, k = coeffs(in_size, out_size)
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + a.shape[1:], np.int64)
    for o in range(out_size):
        xmin, cnt = int(bounds[o, 0]), int(bounds[o, 1])
        s = np.tensordot(k[o, :cnt].astype(np.int64), a[xmin:xmin + cnt], axes=(0, 0))
        out[o] = s
    out = np.clip((out + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def vertical_first(h, w):
    """the pass order of the installed Pillow: vertical first only for h > 100 w"""
    return h > 100 * w


def resize(rgb, size=(192, 280)):
    """uint8 (n, h, w, 3) or (h, w, 3) -> the same with (H, W) = size"""
    rgb = np.asarray(rgb, np.uint8)
    single = rgb.ndim == 3
    a = rgb[None] if single else rgb
    H, W = size
    h, w = a.shape[1:3]
    if vertical_first(h, w):
        if H != h:
            a = _pass(a, 1, H)
        if W != w:
            a = _pass(a, 2, W)
    else:
        if W != w:
            a = _pass(a, 2, W)
        if H != h:
            a = _pass(a, 1, H)
    a = np.ascontiguousarray(a)
    return a[0] if single else a


def pillow_resize(rgb, size=(192, 280)):
    """PIL.Image.resize((W, H), LANCZOS) of every frame (needs Pillow)"""
    from PIL import Image
    rgb = np.asarray(rgb, np.uint8)
    single = rgb.ndim == 3
    a = rgb[None] if single else rgb
    out = np.stack([np.asarray(Image.fromarray(f).resize((size[1], size[0]), resample=Image.LANCZOS)) for f in a])
    return out[0] if single else out


def sizes(seed=1234, n_random=100):
    """the (h, w, H, W) cases the tests pin"""
    fixed = [(480, 640, 192, 280), (1080, 1920, 192, 280), (720, 1280, 192, 280),
             (37, 53, 192, 280), (96, 140, 192, 280),
             (192, 1000, 192, 280), (720, 280, 192, 280),
             (1, 1, 192, 280), (1, 2000, 192, 280), (2000, 1, 192, 280),
             (400, 4, 192, 280), (401, 4, 192, 280), (300, 3, 17, 9), (301, 3, 17, 9),
             (192, 280, 192, 280), (5, 7, 3, 2)]
    rng = np.random.RandomState(seed)
    rand = []
    for _ in range(n_random):
        h, w = (int(v) for v in rng.randint(1, 400, size=2))
        H, W = (int(v) for v in rng.randint(1, 300, size=2))
        rand.append((h, w, H, W))
    return fixed, rand
