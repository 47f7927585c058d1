"""The tests' model of f12 (include/iivision.h: iiv_resize_coeffs_box / iiv_resize_frames_fit / iiv_resize_frames_yuv420_fit;
DESIGN.md 28), written in numpy from that text on top of resize_model: Pillow's Image.resize((rw, rh), LANCZOS, box=box) pasted
at (rx, ry) onto a canvas of the fill colour.

    the box        four float32 values; scale = (double)(in1 - in0) / out with the subtraction in float32
    coefficients   center = in0 + (xx + 0.5) scale; the rest as resize_model.coeffs, clamped at the axis, not at the box
    passes         an axis gets one when out != in or the box does not span it; horizontal first, vertical first when the
                   frame has h > 100 w
    canvas         the fill colour outside the rectangle

and a restatement of frame_grabber.fit_geometry (letterbox and crop on a 4:3 screen) in its own words.
"""
import math
from fractions import Fraction

import numpy as np

import resize_model as RM

PRECISION_BITS = RM.PRECISION_BITS


def coeffs_box(in_size, in0, in1, out_size):
    """-> (ksize, bounds int32 (out, 2) = (xmin, count), fixed-point int32 (out, ksize), zero past count)"""
    in0, in1 = np.float32(in0), np.float32(in1)
    extent = in1 - in0
    assert extent.dtype == np.float32
    scale = filterscale = float(extent) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = RM.SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = float(in0) + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [RM.lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, k


def _pass(a, axis, in0, in1, out_size):
    """one pass of uint8 (n, h, w, 3) along axis 1 (vertical) or 2 (horizontal) over the box [in0, in1) of that axis"""
    _, bounds, k = coeffs_box(a.shape[axis], in0, in1, out_size)
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + a.shape[1:], np.int64)
    for o in range(out_size):
        xmin, cnt = int(bounds[o, 0]), int(bounds[o, 1])
        out[o] = np.tensordot(k[o, :cnt].astype(np.int64), a[xmin:xmin + cnt], axes=(0, 0))
    out = np.clip((out + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize_box(rgb, box, size):
    """uint8 (n, h, w, 3) or (h, w, 3), box (x0, y0, x1, y1), size (rh, rw) -> Image.resize((rw, rh), LANCZOS, box=box)"""
    rgb = np.asarray(rgb, np.uint8)
    single = rgb.ndim == 3
    a = rgb[None] if single else rgb
    x0, y0, x1, y1 = (np.float32(v) for v in box)
    rh, rw = size
    h, w = a.shape[1:3]
    horizontal = rw != w or x0 != 0 or x1 != w
    vertical = rh != h or y0 != 0 or y1 != h
    order = (1, 2) if RM.vertical_first(h, w) else (2, 1)
    for axis in order:
        if axis == 2 and horizontal:
            a = _pass(a, 2, x0, x1, rw)
        if axis == 1 and vertical:
            a = _pass(a, 1, y0, y1, rh)
    a = np.ascontiguousarray(a)
    return a[0] if single else a


def fit(rgb, box, size, rect, fill):
    """the whole destination: uint8 (n, H, W, 3) (or (H, W, 3)), size = (H, W), rect = (rx, ry, rw, rh), fill = (r, g, b)"""
    rgb = np.asarray(rgb, np.uint8)
    H, W = size
    rx, ry, rw, rh = rect
    inner = resize_box(rgb, box, (rh, rw))
    out = np.empty(rgb.shape[:-3] + (H, W, 3), np.uint8)
    out[...] = np.array(fill, np.uint8)
    out[..., ry:ry + rh, rx:rx + rw, :] = inner
    return out


def pillow_fit(rgb, box, size, rect, fill):
    """the same from Pillow itself: resize(box=) and paste onto a filled canvas (needs Pillow)"""
    from PIL import Image
    rgb = np.asarray(rgb, np.uint8)
    single = rgb.ndim == 3
    H, W = size
    rx, ry, rw, rh = rect
    out = []
    for f in (rgb[None] if single else rgb):
        canvas = Image.new("RGB", (W, H), tuple(int(c) for c in fill))
        canvas.paste(Image.fromarray(f).resize((rw, rh), resample=Image.LANCZOS, box=tuple(float(v) for v in box)), (rx, ry))
        out.append(np.asarray(canvas))
    return out[0] if single else np.stack(out)


def _half_up(q):
    return int(math.floor(q + Fraction(1, 2)))


def fit_geometry(h, w, H, W, fit, sar=(1, 1)):
    """frame_grabber.fit_geometry restated: the screen shows a 4:3 picture whatever H and W are, so only the source's display
    aspect against 4:3 matters -> (box as four float32-exact floats, rect as four ints)"""
    whole = ((0.0, 0.0, float(w), float(h)), (0, 0, W, H))
    ratio = Fraction(w * sar[0], h * sar[1]) / Fraction(4, 3)   # > 1: the source is wider than the screen
    if fit == "stretch" or ratio == 1:
        return whole
    if fit == "letterbox":
        if ratio > 1:
            rw, rh = W, max(_half_up(H / ratio), 1)
        else:
            rw, rh = min(max(2 * _half_up(W * ratio / 2), 2), W), H
        return whole[0], ((W - rw) // 2, (H - rh) // 2, rw, rh)
    assert fit == "crop"
    if ratio > 1:
        bw = Fraction(w) / ratio
        box = ((w - bw) / 2, Fraction(0), (w + bw) / 2, Fraction(h))
    else:
        bh = Fraction(h) * ratio
        box = (Fraction(0), (h - bh) / 2, Fraction(w), (h + bh) / 2)
    return tuple(float(np.float32(float(v))) for v in box), whole[1]
