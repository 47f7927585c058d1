"""numpy restatement of iiv_render_error's contract (include/iivision.h, "f8: screen error") on top of render_model.render_rgb:
the screen f7 draws against a reference picture, as exact integer sums of squared differences.  Written from the contract's
words, int64 throughout; it takes nothing from the kernel or the library.

S is the rendered screen (192 x 560 x 3), R the reference brought to 560 wide (R[x] = ref[x * ref_width // 560], ref_width
560 or 280), D = S - R.  Per frame and channel: level 0 sums D^2 over the dots, level 1 adds the D of each quad of four dots
of a row before squaring (140 quads per row), level 2 those of each unit of sixteen dots (35 per row)."""
import numpy as np

import render_model as R

CELLS = (107520, 26880, 6720)     # blocks per frame and channel: 192 x 560, 192 x 140, 192 x 35
BLOCK = (1, 4, 16)                # dots per block


def widen(ref):
    """(..., 192, W, 3), W = 560 or 280 -> (..., 192, 560, 3): R[x] = ref[x * W // 560]"""
    ref = np.asarray(ref)
    w = ref.shape[-2]
    assert w in (280, 560) and ref.shape[-3] == 192 and ref.shape[-1] == 3
    return ref[..., (np.arange(R.WIDTH) * w) // R.WIDTH, :]


def error_sums_of_screens(screen_rgb, ref):
    """screen_rgb (n, 192, 560, 3) u8, ref (n, 192, 560 or 280, 3) u8 -> (n, 3, 3) uint64 [frame][level][channel]"""
    d = np.asarray(screen_rgb).astype(np.int64) - widen(ref).astype(np.int64)          # (n, 192, 560, 3)
    n = d.shape[0]
    out = np.zeros((n, 3, 3), dtype=np.int64)
    for level, k in enumerate(BLOCK):
        blocks = d.reshape(n, 192, R.WIDTH // k, k, 3).sum(axis=3)                      # every block lies in one row
        out[:, level, :] = (blocks * blocks).sum(axis=(1, 2))
    return out.astype(np.uint64)


def render_error(mode, main, aux, palette_rgb, ref):
    """(n, 32, 256) memory maps, a (16, 3) palette, ref (n, 192, 560 or 280, 3) -> (n, 3, 3) uint64"""
    return error_sums_of_screens(R.render_rgb(mode, main, aux, palette_rgb), ref)


def psnr(sums, level):
    """(..., 3, 3) sums -> (per channel (..., 3), overall (...)) in dB, float64; inf for a zero sum:
    10 log10(255^2 * cells * k^2 / sum), cells and k of the level; overall with three times the cells over the channels' total"""
    e = np.asarray(sums)[..., level, :].astype(np.float64)
    peak = 255.0 ** 2 * CELLS[level] * BLOCK[level] ** 2
    tot = e.sum(axis=-1)
    with np.errstate(divide="ignore"):
        return 10 * np.log10(peak / e), 10 * np.log10(3 * peak / tot)
