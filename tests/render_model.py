"""numpy restatement of iiv_render_rgb's contract (include/iivision.h, "f7: preview"): screen memory -> 560 x 192 colour
values -> RGB.  Written from the contract's words; it takes nothing from the kernel or the library.

A screen row is 560 dots.  DHGR: the row's bytes aux[0], main[0], aux[1], main[1], ... give seven dots each (bits 0..6).
HGR: a byte's seven data bits give two dots each, shifted one dot right when its palette bit (bit 7) is set; the dot the
shift uncovers is bit 6 of the byte to the left (0 at the row's start), the 561st dot is dropped.  The colour value of dot x
is the window of dots x - 3 .. x (dots left of the row are 0) rotated left by (x + 1) & 3 -- the reference's sliding window
(colours.py:100-134) per screen row -- and a pixel is palette_rgb[value]."""
import numpy as np

HGR, DHGR = 0, 1
WIDTH, HEIGHT = 560, 192


def y_to_offset(y):
    """y_to_base_addr(y) - 0x2000 (screen.py:16-22): where row y's 40 bytes start in an 8 KiB memory map"""
    return 1024 * (y % 8) + 128 * ((y % 64) // 8) + 40 * (y // 64)


ROW_OFFSET = np.array([y_to_offset(y) for y in range(HEIGHT)])


def rol4(v, n):
    """colours.py:87-97: a 4-bit value rotated left n times"""
    for _ in range(n):
        v = ((v & 0b0111) << 1) ^ ((v & 0b1000) >> 3)
    return v


ROL4 = np.array([[rol4(v, n) for n in range(4)] for v in range(16)], dtype=np.uint8)   # [value][times]


def rows_of(mem):
    """(..., 32, 256) memory maps -> (..., 192, 40): the bytes of every screen row (the screen holes are never looked at)"""
    flat = np.asarray(mem, dtype=np.uint8).reshape(mem.shape[:-2] + (8192,))
    return flat[..., ROW_OFFSET[:, None] + np.arange(40)[None, :]]


def dots(mode, main, aux=None):
    """(..., 192, 560) uint8 0 / 1"""
    m = rows_of(main)
    if mode == DHGR:
        a = rows_of(aux)
        seq = np.stack([a, m], axis=-1).reshape(m.shape[:-1] + (80,))             # aux[0], main[0], aux[1], ...
        return ((seq[..., None] >> np.arange(7)) & 1).reshape(m.shape[:-1] + (WIDTH,)).astype(np.uint8)
    x = np.arange(WIDTH)
    i, r = x // 14, x % 14
    byte = m[..., i]
    left = np.concatenate([np.zeros_like(m[..., :1]), m[..., :-1]], axis=-1)[..., i]   # byte i - 1, 0 for i = 0
    plain = (byte >> (r // 2)) & 1
    shifted = np.where(r > 0, (byte >> (np.maximum(r, 1) - 1) // 2) & 1, (left >> 6) & 1)
    return np.where(byte >> 7 == 0, plain, shifted).astype(np.uint8)


def colour_values(mode, main, aux=None):
    """(..., 192, 560) uint8 colour values 0..15"""
    d = dots(mode, main, aux)
    p = np.concatenate([np.zeros(d.shape[:-1] + (3,), np.uint8), d], axis=-1)     # p[x + 3] = d[x]
    w = p[..., 0:WIDTH] | (p[..., 1:WIDTH + 1] << 1) | (p[..., 2:WIDTH + 2] << 2) | (p[..., 3:WIDTH + 3] << 3)
    return ROL4[w, (np.arange(WIDTH) + 1) & 3]


def render_rgb(mode, main, aux, palette_rgb):
    """(..., 192, 560, 3) uint8"""
    pal = np.asarray(palette_rgb, dtype=np.uint8).reshape(16, 3)
    return pal[colour_values(mode, main, aux)]


# ---- the bytes a row of one aligned repeating dot quad P takes (dot X = bit X & 3 of P)

def dhgr_quad_row(P):
    """(aux[40], main[40]): the packing iiv_frames_to_memory_maps' contract gives -- seven dots per byte, aux / main alternating"""
    d = (P >> (np.arange(WIDTH) & 3)) & 1
    seq = (d.reshape(80, 7) << np.arange(7)).sum(axis=1).astype(np.uint8)
    return seq[0::2], seq[1::2]


def hgr_quad_row(P, palette_bit):
    """main[40] of an HGR row whose data bits light the dots of quad P as far as HGR can: bit k of a byte is dots 2k, 2k + 1
    (palette bit 0) or 2k + 1, 2k + 2 (palette bit 1) of its fourteen"""
    first = np.arange(40)[:, None] * 14 + 2 * np.arange(7)[None, :] + palette_bit     # the first dot bit k lights
    bits = (P >> (first & 3)) & 1
    return ((bits << np.arange(7)).sum(axis=1) | (palette_bit << 7)).astype(np.uint8)
