"""CPU: tests/render_model.py -- the numpy restatement of iiv_render_rgb's contract -- against the reference's own colour
model: the colour strings the reference computed for every masked value (tests/golden/g2_dots_pixels.npz:
HGRBitmap / DHGRBitmap.to_dots + colours.dots_to_nominal_colour_pixel_values with the modes' PHASES), the aligned-quad rule
iiv_frames_to_memory_maps promises, and the one place where the contract leaves the reference: a row starts with no dots to
its left."""
import numpy as np
import pytest

import render_model as R

# screen.py:632-636, 894-910: BYTE_MASKS / BYTE_SHIFTS of the packed columns; MASKED_DOTS
MASKS = {R.HGR: [0x3fff, 0x3fff << 8], R.DHGR: [0x1fff << (7 * k) for k in range(4)]}
SHIFTS = {R.HGR: [0, 8], R.DHGR: [0, 7, 14, 21]}
MASKED_DOTS = {R.HGR: 18, R.DHGR: 10}
NAME = {R.HGR: "HGR", R.DHGR: "DHGR"}


def _random_screen(rng):
    """every byte random, the screen holes too"""
    return rng.integers(0, 256, (32, 256), dtype=np.uint8)


@pytest.mark.parametrize("mode", [R.HGR, R.DHGR])
def test_model_shows_the_reference_recorded_strings(O, golden, mode):
    """Every byte that is neither first nor last in its row: packed by the oracle's pack, masked and shifted as
    Bitmap.mask_and_shift_data does, its masked value's recorded string is what the model shows from the byte's first dot on."""
    pix = golden.g2_dots_pixels[NAME[mode] + "_pixels"]
    page, offset = O.xy_tables()                      # (192, 40) each
    nd = MASKED_DOTS[mode]
    rng = np.random.default_rng(20 + mode)
    seen = set()
    for _ in range(2):
        main, aux = _random_screen(rng), _random_screen(rng)
        packed = O.pack(mode, main, aux if mode == R.DHGR else None)
        values = R.colour_values(mode, main, aux if mode == R.DHGR else None)
        rows = R.rows_of(main)
        ys = np.arange(192)[:, None]
        if mode == R.DHGR:
            b = np.arange(1, 79)[None, :]             # index in the row's 80-byte sequence aux[0], main[0], aux[1], ...
            col, is_aux = b // 2, b % 2 == 0
            bo = 2 * (offset[ys, col] & 1) + np.where(is_aux, 0, 1)
            x0 = 7 * b
        else:
            b = np.arange(1, 39)[None, :]
            col = b
            bo = offset[ys, col] & 1
            x0 = 14 * b
        column = packed[page[ys, col], offset[ys, col] // 2]
        m = (column & np.array(MASKS[mode], np.uint64)[bo]) >> np.array(SHIFTS[mode], np.uint64)[bo]
        want = pix[bo, m.astype(np.int64)]                                      # (192, bytes, nd)
        got = values[ys[:, :, None], (x0 + np.zeros_like(ys))[:, :, None] + np.arange(nd)[None, None, :]]
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "row %d, byte %d, dot %d of its string: model %d, reference %d" % (
            bad[0][0], b[0, bad[0][1]], bad[0][2], got[tuple(bad[0])], want[tuple(bad[0])])
        if mode == R.DHGR:
            seen |= set(np.unique(bo).tolist())
        else:
            p = rows >> 7
            for o in (0, 1):
                at = np.argwhere(bo == o)
                seen |= {(o, int(p[y, b[0, k] - 1]), int(p[y, b[0, k]]), int(p[y, b[0, k] + 1])) for y, k in at}
    if mode == R.DHGR:
        assert seen == {0, 1, 2, 3}
    else:   # both byte offsets, with both values of the palette bit on the byte and on each side of it
        assert seen == {(o, a, c, e) for o in (0, 1) for a in (0, 1) for c in (0, 1) for e in (0, 1)}


def _map_with_row(y, row_bytes, fill=0):
    mem = np.full(8192, fill, np.uint8)
    o = R.y_to_offset(y)
    mem[o:o + 40] = row_bytes
    return mem.reshape(32, 256)


@pytest.mark.parametrize("P", range(16))
def test_an_aligned_repeating_quad_shows_its_own_value_dhgr(P):
    """iiv_frames_to_memory_maps: "a repeating quad P shows colour value P" -- through the bytes its packing gives"""
    a, m = R.dhgr_quad_row(P)
    for y in (0, 77, 191):
        v = R.colour_values(R.DHGR, _map_with_row(y, m), _map_with_row(y, a))
        assert (v[y, 3:] == P).all()
        assert (v[np.arange(192) != y] == 0).all()


@pytest.mark.parametrize("P,palette_bit", [(0, 0), (3, 0), (12, 0), (15, 0), (0, 1), (6, 1), (9, 1), (15, 1)])
def test_an_aligned_repeating_quad_shows_its_own_value_hgr(P, palette_bit):
    """The quads HGR can light: pairs of equal dots, on even columns (palette bit 0: black, violet 3, green 12, white) or odd
    ones (palette bit 1: blue 6, orange 9).  With the palette bit set dot 0 of a row is always dark, so orange -- whose quad
    lights dot 0 -- shows from dot 4 on: the first window that does not hold dot 0."""
    v = R.colour_values(R.HGR, _map_with_row(100, R.hgr_quad_row(P, palette_bit)))
    first = 4 if palette_bit and P & 1 else 3
    assert (v[100, first:] == P).all()


@pytest.mark.parametrize("mode", [R.HGR, R.DHGR])
def test_a_row_starts_with_no_dots_to_its_left(mode):
    """Dots 0..2 of a row are windows over the dots left of the row, which are 0 -- not, as in the reference's packed
    form (screen.py:190, a TODO there), the last byte of whatever precedes the row in its page."""
    rng = np.random.default_rng(5)
    main, aux = _random_screen(rng), _random_screen(rng)
    base = R.colour_values(mode, main, aux)
    d = R.dots(mode, main, aux)
    # from the row's own dots alone
    for x in range(3):
        w = sum(int(d[9, x - 3 + k]) << k for k in range(4) if x - 3 + k >= 0)
        assert base[9, x] == R.rol4(w, (x + 1) & 3)
    # the last byte of the previous row in the same page: rows 0 and 64 share page 0 (offsets 0..39 and 40..79)
    assert R.y_to_offset(64) == R.y_to_offset(0) + 40
    m2, a2 = main.copy(), aux.copy()
    m2[0, 39] ^= 0xff
    a2[0, 39] ^= 0xff
    other = R.colour_values(mode, m2, a2)
    assert (other[64] == base[64]).all() and (other[1:] == base[1:]).all()
    assert (other[0] != base[0]).any()
    # the screen holes are never looked at
    holes = (np.arange(256) & 127) >= 120
    m3, a3 = main.copy(), aux.copy()
    m3[:, holes] = 0xff
    a3[:, holes] = 0xff
    assert (R.colour_values(mode, m3, a3) == base).all()
    # HGR does not look at aux at all
    if mode == R.HGR:
        assert (R.colour_values(mode, main, None) == base).all()


@pytest.mark.parametrize("p_i,p_next", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_hgr_palette_bits_around_a_set_bit_6(p_i, p_next):
    """Byte i has bit 6 set.  Its own palette bit decides whether bit 6 lights dots 12, 13 or only 13 of its fourteen; the
    first dot of byte i + 1 is that byte's bit 0 (p_{i+1} = 0) or byte i's bit 6 (p_{i+1} = 1)."""
    for bit0_next in (0, 1):
        row = np.zeros(40, np.uint8)
        i = 17
        row[i] = 0x40 | (p_i << 7)
        row[i + 1] = bit0_next | (p_next << 7)
        d = R.dots(R.HGR, _map_with_row(3, row))[3]
        x0 = 14 * i
        want = np.zeros(560, np.uint8)
        if p_i == 0:
            want[x0 + 12] = want[x0 + 13] = 1
        else:
            want[x0 + 13] = 1
        if p_next == 0:
            want[x0 + 14] = want[x0 + 15] = bit0_next
        else:
            want[x0 + 14] = 1                      # bit 6 of byte i
            want[x0 + 15] = want[x0 + 16] = bit0_next
        assert (d == want).all()
    # ... and at the row's start there is no byte to the left: dot 0 is dark
    row = np.zeros(40, np.uint8)
    row[0] = 0x80 | 0x01
    d = R.dots(R.HGR, _map_with_row(3, row))[3]
    assert d[0] == 0 and d[1] == 1 and d[2] == 1 and d[3:].sum() == 0
    # ... and the 561st dot a shifted last byte would light is dropped
    row = np.zeros(40, np.uint8)
    row[39] = 0x80 | 0x40
    d = R.dots(R.HGR, _map_with_row(3, row))[3]
    assert d.shape == (560,) and d[559] == 1 and d[:559].sum() == 0
