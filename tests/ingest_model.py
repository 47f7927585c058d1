"""The colour RGB -> memory-map conversion, restated in numpy from its contract (include/iivision.h: the comment of
iiv_frames_to_memory_maps).  The yardstick of oracle.frame_to_memory_map and, through it, of csrc/iiv_ingest.hip: written
from the contract, not from the oracle's C or the kernels.  The colour distance is computed as it is written,
2 dr^2 + 4 dg^2 + 3 db^2 in int64, and a tie is whatever numpy's argmin makes of equal distances: the first, i.e. the
lower colour value / the lower pattern.

    frame_to_memory_map(mode, palette_rgb, rgb, dither)      one frame -> (main, aux | None), (32, 256) uint8
    frames_to_memory_maps(mode, palettes, rgb, dither)       B frames, frame i under palettes[i] -> (B, 32, 256) each
    unpack(mode, main, aux)                                  one frame's dots back out of the bytes: (192, 560 | 280)
    PALETTES, frame_set(palette, seed)                       the adversarial palettes and the frames the tests share
    NAMES, palette(O, name), frames_of(O, name)              the sweep of the CPU and GPU tests: those and the two real palettes
One sentence of the contract was read closely: in HGR's ordered path "dot X = .. the pattern of pixel X >> 1 under that palette
bit" is taken per DOT -- the pixel that straddles two screen bytes gives each byte its dot under that byte's own bit (in the
diffusion path the contract says outright that a pixel has one pattern, under the bit of the byte holding its first dot).
The oracle reads it the same way; the header was left as it is (the library's build id is a hash that includes it).
The ordered dither is vectorised over the frame; error diffusion is the contract's raster-order loop over the 140 x 192
colour pixels, each step taken for all B frames at once (integers throughout).
"""
import numpy as np

HGR, DHGR = 0, 1
DITHER_DIFFUSION = 256
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], dtype=np.int64)
WEIGHT = np.array([2, 4, 3], dtype=np.int64)                 # 2 dr^2 + 4 dg^2 + 3 db^2
HGR_COLOURS = np.array([[0, 3, 12, 15], [0, 6, 9, 15]])      # [palette bit][2-dot pattern]: black, violet | blue, green | orange, white


def y_to_offset(y):
    """y_to_base_addr(y, 0) - 0x2000 (screen.py:16-22)"""
    a, d = divmod(y, 64)
    b, c = divmod(d, 8)
    return 1024 * c + 128 * b + 40 * a


def colour_pixels(rgb):
    """(..., 192, 280, 3) uint8 -> (..., 192, 140, 3) int64: source pixels 2k, 2k + 1 averaged, (a + b + 1) / 2"""
    rgb = np.asarray(rgb).astype(np.int64)
    return (rgb[..., 0::2, :] + rgb[..., 1::2, :] + 1) // 2


def distance(v, colours):
    """v (..., 3), colours (..., m, 3) -> (..., m): the contract's colour distance, literally"""
    d = v[..., None, :] - colours
    return (WEIGHT * d * d).sum(axis=-1)


def bayer_offset(dither):
    """(192, 140) ordered-dither offsets: floor((2 B[y & 3][k & 3] - 15) * dither / 16)"""
    off = np.floor_divide((2 * BAYER - 15) * int(dither), 16)
    return off[np.arange(192)[:, None] & 3, np.arange(140)[None, :] & 3]


# ---- dots -> bytes ---------------------------------------------------------------------------

def _place(rowbytes):
    """(B, 192, 40) row bytes -> (B, 32, 256) memory map, rows at y_to_base_addr, everything else (the holes) zero"""
    mem = np.zeros((rowbytes.shape[0], 8192), dtype=np.uint8)
    for y in range(192):
        o = y_to_offset(y)
        mem[:, o:o + 40] = rowbytes[:, y]
    return mem.reshape(-1, 32, 256)


def _bytes_of(dots):
    """(B, 192, W) dots -> (B, 192, W / 7): dot X = bit X % 7 of byte X / 7 of the row"""
    B, H, W = dots.shape
    return (dots.reshape(B, H, W // 7, 7).astype(np.int64) << np.arange(7)).sum(axis=3)


def pack_dhgr(quads):
    """(B, 192, 140) colour values -> (main, aux): dot X = bit X & 3 of quad X >> 2, seven dots per byte, aux / main
    alternating, bit 7 clear"""
    quads = np.asarray(quads).astype(np.int64)
    dots = ((quads[..., None] >> np.arange(4)) & 1).reshape(quads.shape[0], 192, 560)
    by = _bytes_of(dots)
    return _place(by[:, :, 1::2]), _place(by[:, :, 0::2])


def pack_hgr(dots, pbit):
    """(B, 192, 280) dots, (B, 192, 40) palette bits -> main"""
    return _place(_bytes_of(dots) | (np.asarray(pbit).astype(np.int64) << 7))


def unpack(mode, main, aux=None):
    """One frame's dots, read straight from the bytes: (192, 560) for DHGR, (192, 280) for HGR (bit 7 not included)."""
    m = np.asarray(main).reshape(8192)
    a = np.asarray(aux).reshape(8192) if aux is not None else None
    out = np.zeros((192, 560 if mode == DHGR else 280), dtype=np.uint8)
    for y in range(192):
        o = y_to_offset(y)
        if mode == DHGR:
            row = np.empty(80, dtype=np.uint8)
            row[0::2] = a[o:o + 40]
            row[1::2] = m[o:o + 40]
        else:
            row = m[o:o + 40]
        out[y] = ((row[:, None] >> np.arange(7)) & 1).reshape(-1)
    return out


def rows_of(main):
    """(32, 256) memory map -> (192, 40): the bytes of the 192 rows (i.e. everything but the holes)"""
    m = np.asarray(main).reshape(8192)
    return np.stack([m[y_to_offset(y):y_to_offset(y) + 40] for y in range(192)])


# ---- ordered dither (or none) ----------------------------------------------------------------

def _ordered(mode, pals, mean, dither):
    """pals (B, 16, 3), mean (B, 192, 140, 3) -> (main, aux)"""
    v = np.clip(mean + bayer_offset(dither)[None, :, :, None], 0, 255)
    if mode == DHGR:
        quads = distance(v, pals[:, None, None]).argmin(axis=-1)          # ties: the first = the lower colour value
        return pack_dhgr(quads)
    # HGR: per palette bit and pixel the nearest of the four colours (pattern) and its error
    err, pat = [], []
    for pb in (0, 1):
        d = distance(v, pals[:, HGR_COLOURS[pb]][:, None, None])          # (B, 192, 140, 4)
        pat.append(d.argmin(axis=-1))                                     # ties: the lower pattern
        err.append(d.min(axis=-1))
    pixel_of_dot = np.arange(280) >> 1
    # the error of a dot is its pixel's; a byte's is the sum over its seven dots
    s = [e[:, :, pixel_of_dot].reshape(-1, 192, 40, 7).sum(axis=-1) for e in err]
    pbit = (s[1] < s[0]).astype(np.int64)                                 # the smaller sum, ties to 0
    pb_of_dot = pbit[:, :, np.arange(280) // 7]                           # the palette bit of the byte holding the dot
    patt_of_dot = np.where(pb_of_dot == 1, pat[1][:, :, pixel_of_dot], pat[0][:, :, pixel_of_dot])
    dots = (patt_of_dot >> (np.arange(280) & 1)) & 1                      # pattern bit 0 = the even dot column
    return pack_hgr(dots, pbit), None


# ---- error diffusion --------------------------------------------------------------------------

def _hgr_byte_groups():
    """For every screen byte b of a row: the pixels whose first dot (2k) lies in b and how many of their dots do (2 or 1);
    and for every pixel the byte it opens (-1: none)."""
    groups, opens = [], np.full(140, -1)
    for b in range(40):
        ks = [k for k in range(140) if (2 * k) // 7 == b]
        w = [2 if (2 * k + 1) // 7 == b else 1 for k in ks]
        groups.append((np.array(ks), np.array(w, dtype=np.int64)))
        opens[ks[0]] = b
    return groups, opens


def _diffuse(mode, pals, mean):
    """Floyd-Steinberg as the contract words it: rows top to bottom, pixels left to right, sixteenths accumulators."""
    B = mean.shape[0]
    rows = np.arange(B)
    acc = np.zeros((B, 192, 140, 3), dtype=np.int64)
    chosen = np.zeros((B, 192, 140), dtype=np.int64)          # DHGR: colour value; HGR: 2-dot pattern
    pbit = np.zeros((B, 192, 40), dtype=np.int64)
    groups, opens = _hgr_byte_groups()
    four = [pals[:, HGR_COLOURS[0]], pals[:, HGR_COLOURS[1]]]   # (B, 4, 3) per palette bit
    for y in range(192):
        for k in range(140):
            if mode == HGR and opens[k] >= 0:
                # the palette bit of the byte this pixel opens, with the errors accumulated up to now
                b = opens[k]
                ks, w = groups[b]
                vals = np.clip(mean[:, y, ks] + np.floor_divide(acc[:, y, ks], 16), 0, 255)       # (B, m, 3)
                s = [(w * distance(vals, four[pb][:, None]).min(axis=-1)).sum(axis=-1) for pb in (0, 1)]
                pbit[:, y, b] = s[1] < s[0]
            v = np.clip(mean[:, y, k] + np.floor_divide(acc[:, y, k], 16), 0, 255)                  # (B, 3)
            if mode == DHGR:
                c = distance(v, pals).argmin(axis=-1)
                colour = pals[rows, c]
            else:
                pb = pbit[:, y, (2 * k) // 7]                 # of the byte holding the pixel's first dot
                cols = np.where((pb == 1)[:, None, None], four[1], four[0])
                c = distance(v, cols).argmin(axis=-1)
                colour = cols[rows, c]
            chosen[:, y, k] = c
            e = v - colour
            if k + 1 < 140:
                acc[:, y, k + 1] += 7 * e
            if y + 1 < 192:
                if k > 0:
                    acc[:, y + 1, k - 1] += 3 * e
                acc[:, y + 1, k] += 5 * e
                if k + 1 < 140:
                    acc[:, y + 1, k + 1] += e
    if mode == DHGR:
        return pack_dhgr(chosen)
    # bit 0 / 1 of a pixel's pattern go to its first / second dot
    dots = ((chosen[..., None] >> np.arange(2)) & 1).reshape(B, 192, 280)
    return pack_hgr(dots, pbit), None


# ---- the entry points -------------------------------------------------------------------------

def frames_to_memory_maps(mode, palettes, rgb, dither=0):
    """palettes (B, 16, 3) or (16, 3) for all; rgb (B, 192, 280, 3) uint8 -> (main, aux | None), (B, 32, 256) uint8"""
    rgb = np.asarray(rgb)
    assert mode in (HGR, DHGR) and rgb.dtype == np.uint8 and rgb.shape[1:] == (192, 280, 3)
    pals = np.asarray(palettes).astype(np.int64)
    if pals.ndim == 2:
        pals = np.broadcast_to(pals, (len(rgb), 16, 3))
    assert pals.shape == (len(rgb), 16, 3)
    mean = colour_pixels(rgb)
    if int(dither) == DITHER_DIFFUSION:
        return _diffuse(mode, pals, mean)
    if not 0 <= int(dither) <= 255:
        raise ValueError("dither")
    return _ordered(mode, pals, mean, dither)


def frame_to_memory_map(mode, palette_rgb, rgb, dither=0):
    main, aux = frames_to_memory_maps(mode, np.asarray(palette_rgb).reshape(16, 3), np.asarray(rgb)[None], dither)
    return main[0], (aux[0] if aux is not None else None)


# ---- adversarial palettes ---------------------------------------------------------------------
# Any 48 bytes are a legal palette.  Row i = colour value i; HGR shows values 0, 3, 12, 15 (palette bit 0) and 0, 6, 9, 15.

def _pal(rows):
    a = np.array(rows, dtype=np.uint8)
    assert a.shape == (16, 3)
    return a


# sixteen distinct, well separated colours the tie palettes are cut from
_BASE = [(12, 8, 20), (201, 30, 88), (64, 52, 190), (230, 60, 240), (10, 110, 80), (120, 125, 118), (40, 150, 250), (190, 170, 255),
         (90, 75, 5), (245, 120, 30), (135, 130, 140), (255, 160, 200), (30, 215, 25), (210, 220, 120), (100, 240, 190), (250, 252, 246)]

_CORNER = [(255 * (i & 1), 255 * ((i >> 1) & 1), 255 * ((i >> 2) & 1)) for i in range(8)]


def _hgr_ties(black_is_white):
    p = list(_BASE)
    p[6] = p[3]             # blue == violet
    p[9] = p[12]            # orange == green
    if black_is_white:
        p[15] = p[0]
    return _pal(p)


PALETTES = {
    # channels in {0, 255} only: the largest squares and products the distance can take.  Values 0..7 are the eight cube
    # corners (0 black, 7 white), 8..15 the same again (8 black .. 15 white); HGR's six values are six different corners.
    "corners": _pal(_CORNER + _CORNER),
    # every comparison ties: colour value 0 in DHGR, pattern 0 and palette bit 0 in HGR
    "all_equal": _pal([(128, 128, 128)] * 16),
    # value c and value c ^ 8 are the same colour: the lower wins, no chosen value is >= 8
    "pairs": _pal([_BASE[2 * (c & 7)] for c in range(16)]),
    # both palette bits offer the same four colours: every byte's sums tie, the palette bit is always 0
    "hgr_ties": _hgr_ties(False),
    "hgr_ties_bw": _hgr_ties(True),
    # neighbours on the colour lattice, one step in one channel apart: the smallest distance gaps there are (2, 3, 4)
    "neighbours": _pal([(100 + (c & 1) + 2 * (c >> 3), 100 + ((c >> 1) & 1), 100 + ((c >> 2) & 1)) for c in range(16)]),
    # greys 0, 2, .. 30: an odd grey is exactly half way between two entries
    "even_greys": _pal([(2 * c, 2 * c, 2 * c) for c in range(16)]),
    "random_a": np.random.default_rng(20240).integers(0, 256, (16, 3)).astype(np.uint8),
    "random_b": np.random.default_rng(20241).integers(0, 256, (16, 3)).astype(np.uint8),
}

NAMES = list(PALETTES) + ["ntsc", "iigs"]          # the sweep: the palettes above and the two real ones


def palette(O, name):
    """a palette of the sweep by name; the real ones are the oracle module's (O.PALETTE_RGB)"""
    return PALETTES[name] if name in PALETTES else O.PALETTE_RGB[{"ntsc": 5, "iigs": 0}[name]]


def frames_of(O, name):
    """the frame set of a palette of the sweep; the noise frames' seed is the palette's place in NAMES"""
    return frame_set(palette(O, name), 100 + NAMES.index(name))


DITHERS_CPU = (0, 1, 32, 255, DITHER_DIFFUSION)
DITHERS_GPU = (0, 17, 255, DITHER_DIFFUSION)
FRAME_KINDS = ("noise", "odd greys", "checkerboard", "gradient", "own colours", "near colours")


def frame_set(palette, seed):
    """The frames every palette is run on, (6, 192, 280, 3) uint8: uniform noise; odd greys 1..29 (each colour pixel's two
    source pixels alike, so the mean stays odd); a black / white one-pixel checkerboard; a two-axis gradient; the
    palette's own colours in runs of seven colour pixels that start three pixels further left on each row, so every
    screen-byte boundary falls inside a run somewhere; and the palette's colours under noise of -3 .. 3 per channel,
    which keeps the candidates' distances close together whatever the palette."""
    palette = np.asarray(palette, dtype=np.uint8).reshape(16, 3)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:192, 0:280]
    k = x // 2
    out = np.empty((len(FRAME_KINDS), 192, 280, 3), np.uint8)
    out[0] = rng.integers(0, 256, (192, 280, 3))
    out[1] = (2 * ((3 * k + 5 * y) % 15) + 1)[..., None]
    out[2] = (((x + y) & 1) * 255)[..., None]
    out[3] = np.stack([x * 255 // 279, y * 255 // 191, (x + y) * 255 // 470], axis=-1)
    out[4] = palette[((k + 3 * y) // 7) % 16]
    near = palette[rng.integers(0, 16, (192, 140))].astype(np.int64).repeat(2, axis=1) + rng.integers(-3, 4, (192, 280, 3))
    out[5] = np.clip(near, 0, 255)
    return out
