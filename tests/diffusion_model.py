"""The colour conversion's error diffusion with a chosen kernel, restated in numpy from its contract (include/iivision.h: the
comment of iiv_frames_to_memory_maps_diffused).  The yardstick of csrc/iiv_diffuse.hip: written from the contract's words,
not from the kernel.  Everything but the distribution of a pixel's error is ingest_model's, by import: the averaging, the
colour distance as it is written, numpy's argmin for the ties, the byte groups of HGR's palette-bit rule, the packing.

    frames_to_memory_maps(mode, palettes, rgb, weights, divisor)   B frames, frame i under palettes[i] -> (B, 32, 256) each
    check_arguments(weights, divisor)                              the contract's refusals, as a ValueError
    floor_div_constants(divisor), floor_div(acc, divisor)          the multiply-and-shift the contract says is exact
    KERNELS, MADE_UP                                               the named kernels as the issue's table words them
The raster loop is taken for all B frames at once, as ingest_model._diffuse does it (integers throughout).
"""
import numpy as np

import ingest_model as M
from ingest_model import DHGR, HGR, HGR_COLOURS, colour_pixels, distance, pack_dhgr, pack_hgr, _hgr_byte_groups

ACC_MAX = 255 * 64


def _kernel(row0, row1, row2, divisor):
    """row 0 right of the pixel (dx +1, +2), row 1 and row 2 (dx -2 .. +2; None: no such row), the divisor"""
    w = np.zeros((3, 5), dtype=np.int64)
    w[0, 3:] = row0
    if row1 is not None:
        w[1] = row1
    if row2 is not None:
        w[2] = row2
    return w, divisor


# the table of the issue, cell for cell (NOT read from frame_grabber.DIFFUSION_KERNELS: the tests hold that one to this one)
KERNELS = {
    "floyd-steinberg": _kernel((7, 0), (0, 3, 5, 1, 0), None, 16),
    "jarvis": _kernel((7, 5), (3, 5, 7, 5, 3), (1, 3, 5, 3, 1), 48),
    "stucki": _kernel((8, 4), (2, 4, 8, 4, 2), (1, 2, 4, 2, 1), 42),
    "atkinson": _kernel((1, 1), (0, 1, 1, 1, 0), (0, 0, 1, 0, 0), 8),
    "burkes": _kernel((8, 4), (2, 4, 8, 4, 2), None, 32),
    "sierra": _kernel((5, 3), (2, 4, 5, 4, 2), (0, 2, 3, 2, 0), 32),
    "sierra-2": _kernel((4, 3), (1, 2, 3, 2, 1), None, 16),
    "sierra-lite": _kernel((2, 0), (0, 1, 1, 0, 0), None, 4),
    "buckels": _kernel((2, 1), (0, 1, 2, 1, 0), (0, 0, 1, 0, 0), 8),     # (from memory of bmp2dhr's source: an assumption)
}
# Made-up kernels, all twelve weights non-zero, divisor 64, sum below 64: a weight read at the wrong (dy, dx), or a mirrored
# row, changes the result.  Twelve DISTINCT positive integers sum to at least 1 + .. + 12 = 78, more than any legal divisor,
# so one kernel cannot hold twelve different weights; each of these two holds ten different values (sum 58), and the two
# positions that share a value in one of them differ in the other: between them every pair of positions is told apart.
MADE_UP = [_kernel((9, 2), (1, 7, 10, 4, 6), (3, 8, 5, 1, 2), 64),
           _kernel((3, 8), (5, 1, 2, 9, 4), (6, 2, 7, 10, 1), 64)]


def _positions_told_apart(kernels):
    pos = [(dy, dx) for dy in range(3) for dx in range(5) if (dy, dx) >= (0, 3)]
    return all(any(w[a] != w[b] for w, _ in kernels) for a in pos for b in pos if a != b)


assert all((w[np.nonzero(w)].size, int(w.sum()), d) == (12, 58, 64) for w, d in MADE_UP) and _positions_told_apart(MADE_UP)


def check_arguments(weights, divisor):
    """The contract's refusals; returns the weights as (3, 5) int64."""
    w = np.asarray(weights, dtype=np.int64).reshape(3, 5)
    if not 1 <= int(divisor) <= 64:
        raise ValueError("divisor outside 1..64")
    if (w < 0).any() or (w > 255).any():
        raise ValueError("a weight is no byte")
    if w[0, :3].any():
        raise ValueError("a weight on the pixel itself or left of it on its row")
    if w.sum() > divisor:
        raise ValueError("the weights sum to more than the divisor")
    return w


def floor_div_constants(divisor):
    """(bias, multiplier, shift, bias / divisor): floor(acc / divisor) = (((acc + bias) * multiplier) >> shift) - bias / divisor
    for |acc| <= 255 * 64, with acc + bias in 0 .. 2^15 - 1, the multiplier below 2^24 and the product below 2^32 (one 24-bit
    multiply): bias = the multiple of the divisor at or above 255 * 64, shift = 15 + ceil(log2 divisor), multiplier =
    ceil(2^shift / divisor)."""
    d = int(divisor)
    shift = 15 + (d - 1).bit_length()
    mul = -((-1 << shift) // d)
    bias_q = -(-ACC_MAX // d)
    return bias_q * d, mul, shift, bias_q


def floor_div(acc, divisor):
    bias, mul, shift, bias_q = floor_div_constants(divisor)
    return (((np.asarray(acc, dtype=np.int64) + bias) * mul) >> shift) - bias_q


def _diffuse(mode, pals, mean, w, divisor):
    """rows top to bottom, pixels left to right: value = clamp(mean + floor(acc / divisor)), e = value - chosen colour,
    acc[y + dy][k + dx] += w[dy][dx + 2] * e, targets outside the picture dropped (they land in the margin of `acc`)"""
    B = mean.shape[0]
    rows = np.arange(B)
    acc = np.zeros((B, 192 + 2, 140 + 4, 3), dtype=np.int64)      # acc[:, y, k + 2] is pixel (y, k)
    chosen = np.zeros((B, 192, 140), dtype=np.int64)              # DHGR: colour value; HGR: 2-dot pattern
    pbit = np.zeros((B, 192, 40), dtype=np.int64)
    groups, opens = _hgr_byte_groups()
    four = [pals[:, HGR_COLOURS[0]], pals[:, HGR_COLOURS[1]]]     # (B, 4, 3) per palette bit
    spread = [w[dy][None, :, None] for dy in range(3) if w[dy].any()]
    dys = [dy for dy in range(3) if w[dy].any()]
    for y in range(192):
        for k in range(140):
            if mode == HGR and opens[k] >= 0:
                # the palette bit of the byte this pixel opens, with the errors accumulated up to now
                b = opens[k]
                ks, wt = groups[b]
                vals = np.clip(mean[:, y, ks] + np.floor_divide(acc[:, y, ks + 2], divisor), 0, 255)   # (B, m, 3)
                s = [(wt * distance(vals, four[pb][:, None]).min(axis=-1)).sum(axis=-1) for pb in (0, 1)]
                pbit[:, y, b] = s[1] < s[0]
            v = np.clip(mean[:, y, k] + np.floor_divide(acc[:, y, k + 2], divisor), 0, 255)            # (B, 3)
            if mode == DHGR:
                c = distance(v, pals).argmin(axis=-1)
                colour = pals[rows, c]
            else:
                pb = pbit[:, y, (2 * k) // 7]                 # of the byte holding the pixel's first dot
                cols = np.where((pb == 1)[:, None, None], four[1], four[0])
                c = distance(v, cols).argmin(axis=-1)
                colour = cols[rows, c]
            chosen[:, y, k] = c
            e = (v - colour)[:, None, :]
            for dy, sp in zip(dys, spread):
                acc[:, y + dy, k:k + 5] += sp * e             # dx = -2 .. +2 -> columns k .. k + 4 of the padded rows
    # what the picture's own pixels accumulated never left the range the contract promises the kernel
    assert np.abs(acc[:, :192, 2:142]).max(initial=0) <= ACC_MAX
    if mode == DHGR:
        return pack_dhgr(chosen)
    dots = ((chosen[..., None] >> np.arange(2)) & 1).reshape(B, 192, 280)
    return pack_hgr(dots, pbit), None


def frames_to_memory_maps(mode, palettes, rgb, weights, divisor):
    """palettes (B, 16, 3) or (16, 3) for all; rgb (B, 192, 280, 3) uint8 -> (main, aux | None), (B, 32, 256) uint8"""
    rgb = np.asarray(rgb)
    assert mode in (HGR, DHGR) and rgb.dtype == np.uint8 and rgb.shape[1:] == (192, 280, 3)
    w = check_arguments(weights, divisor)
    pals = np.asarray(palettes).astype(np.int64)
    if pals.ndim == 2:
        pals = np.broadcast_to(pals, (len(rgb), 16, 3))
    assert pals.shape == (len(rgb), 16, 3)
    return _diffuse(mode, pals, colour_pixels(rgb), w, int(divisor))
