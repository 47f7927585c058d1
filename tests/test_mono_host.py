"""CPU: mono playback mode's host side -- the cost matrix, the palette surface, and tests/mono_model.py (the yardstick of
csrc/iiv_mono.hip) against the pinned oracle's packing and against itself."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mono_model as M

MODES = [M.DHGR, M.HGR]
DITHERS = [0, 32, 255, M.DITHER_DIFFUSION]


def test_diff_matrix_is_the_formula_and_a_metric():
    import palette
    dm = palette.MonoPalette.diff_matrix()
    assert dm.dtype == np.int32 and dm.shape == (16, 16)
    pc = [bin(v).count("1") for v in range(16)]
    for a in range(16):
        for b in range(16):
            assert dm[a, b] == 16 * abs(pc[a] - pc[b]) + 8 * bin(a ^ b).count("1")
    assert np.array_equal(dm, M.dm_mono())
    assert np.array_equal(dm, dm.T) and (np.diag(dm) == 0).all()
    off = dm[~np.eye(16, dtype=bool)]
    assert off.min() == 16 and off.max() == 96
    for a, b, c in itertools.product(range(16), repeat=3):
        assert dm[a, c] <= dm[a, b] + dm[b, c]
    assert np.array_equal(palette.diff_matrix(palette.Palette.MONO), dm)


def test_palette_surface():
    import palette
    assert set(palette.PALETTES) == {palette.Palette.IIGS, palette.Palette.NTSC}   # make_data_tables.main() iterates it
    assert palette.Palette.MONO.value not in (0, 1, 2, 3, 4, 5) and palette.MonoPalette.ID == palette.Palette.MONO
    assert palette.palette_class(palette.Palette.MONO) is palette.MonoPalette
    assert palette.palette_class(palette.Palette.NTSC) is palette.NTSCPalette
    rgb = palette.MonoPalette.rgb_array()
    for v in range(16):
        assert tuple(rgb[v]) == (int(round(255 * bin(v).count("1") / 4)),) * 3


def test_frame_grabber_takes_one_pixel_per_dot():
    import frame_grabber
    import palette
    from video_mode import VideoMode
    g = frame_grabber.ArrayFrameGrabber(np.zeros((1, 192, 560, 3), np.uint8), VideoMode.DHGR, palette.Palette.MONO)
    assert g.frame_size == (192, 560)
    g = frame_grabber.ArrayFrameGrabber(np.zeros((1, 192, 280, 3), np.uint8), VideoMode.HGR, palette.Palette.MONO)
    assert g.frame_size == (192, 280)
    with pytest.raises(ValueError):
        frame_grabber.ArrayFrameGrabber(np.zeros((1, 192, 280, 3), np.uint8), VideoMode.DHGR, palette.Palette.MONO)
    assert frame_grabber.ArrayFrameGrabber(np.zeros((1, 50, 70, 3), np.uint8), VideoMode.DHGR, palette.Palette.MONO, resize=True).frame_size == (192, 560)
    assert frame_grabber.ArrayFrameGrabber(np.zeros((1, 192, 280, 3), np.uint8), VideoMode.DHGR).frame_size == (192, 280)


def _oracle_dots_of(O, mode, main, aux, y, byte):
    """The dots the oracle reads from screen byte `byte` (0..79 DHGR, 0..39 HGR) of row y: pack, mask, to_dots."""
    L = O.lib()
    pg, po = O.xy_tables()
    packed = O.pack(mode, main, aux)
    col_byte = byte // 2 if mode == M.DHGR else byte          # the byte's offset in its bank's row
    page, off = int(pg[y, col_byte]), int(po[y, col_byte])
    if mode == M.DHGR:
        bo = (0 if byte % 2 == 0 else 1) + (2 if off % 2 else 0)     # aux even / main even / aux odd / main odd: 0 1 2 3
        masked = (int(packed[page, off // 2]) >> (7 * bo)) & 0x1fff
    else:
        bo = off % 2
        masked = (int(packed[page, off // 2]) & (0x3fff if bo == 0 else 0x3fff00)) >> (0 if bo == 0 else 8)
    return int(L.orc_to_dots(mode, C.c_uint32(masked), bo)), packed, page, off


@pytest.mark.parametrize("mode", MODES)
def test_packing_agrees_with_the_oracle(O, mode):
    """A frame with one lit dot X is read back by the oracle's pack + to_dots as exactly that dot."""
    W = M.width(mode)
    xs = [0, 6, 7, 13, 14, 15, 27, 28, W // 2 + 3, W - 15, W - 8, W - 7, W - 1]
    ys = [0, 7, 8, 63, 64, 127, 128, 191]     # both sides of the page boundaries (a page = two rows' bytes)
    for y, X in itertools.product(ys, xs):
        d = np.zeros((1, 192, W), np.uint8)
        d[0, y, X] = 1
        main, aux = M.pack(mode, d)
        assert np.array_equal(M.unpack(mode, main[0], aux[0] if aux is not None else None), d[0])
        got, packed, page, off = _oracle_dots_of(O, mode, main[0], aux[0] if aux is not None else None, y, X // 7)
        if mode == M.DHGR:
            # the masked window of a byte: 3 dots of the byte to its left, its own 7, 3 to its right (to_dots: the identity)
            assert got == 1 << (3 + X % 7), (y, X)
            body = (packed >> np.uint64(3)) & np.uint64((1 << 28) - 1)
            want = np.zeros((32, 128), np.uint64)
            want[page, off // 2] = np.uint64(1) << np.uint64(X % 28)
        else:
            # HGR doubles every dot: dot k of a byte is the window's dots 3 + 2 k, 4 + 2 k (palette bit clear: no shift)
            assert got == 3 << (3 + 2 * (X % 7)), (y, X)
            body = (packed >> np.uint64(3)) & np.uint64(0xffff)
            want = np.zeros((32, 128), np.uint64)
            want[page, off // 2] = np.uint64(1) << np.uint64(X % 14 + (2 if X % 14 >= 7 else 0))   # even byte: bits 0..6, odd byte's data: 9..15
        assert np.array_equal(body, want), (y, X)


@pytest.mark.parametrize("mode", MODES)
def test_black_white_holes_bit7(O, mode):
    """Black stays all-0 and white all-0x7f under error diffusion and under every ordered-dither amplitude whose largest
    offset, floor(15 * dither / 16), stays below the threshold's distance from the ends: dither <= 135 (white: 255 - 127 =
    128 is still lit; black: 0 + 126 is not).  Above that the contract's own formula lights dots on black and clears dots
    on white (amplitude 255: offsets -240 .. 239) -- checked too, over all 256 amplitudes, so that the model is pinned to
    the formula at both ends."""
    W = M.width(mode)
    holes = O.screen_holes()
    rgb = np.zeros((3, 192, W, 3), np.uint8)
    rgb[1] = 255
    rgb[2] = M.noise_frames(mode, 1)[0]
    for dither in (0, 32, 135, 255, M.DITHER_DIFFUSION):
        main, aux = M.frames_to_memory_maps(mode, rgb, dither)
        for bank in ((main, aux) if mode == M.DHGR else (main,)):
            if dither != 255:
                assert (bank[0] == 0).all(), dither
                assert (bank[1][~holes] == 0x7f).all(), dither
            assert (bank[:, holes] == 0).all()
            assert (bank & 0x80 == 0).all()
    assert M.frames_to_memory_maps(M.HGR, np.zeros((1, 192, 280, 3), np.uint8))[1] is None
    black, white = np.zeros((1, 192, W), np.int64), np.full((1, 192, W), 255, np.int64)
    for dither in range(256):
        assert (not M.ordered(black, dither).any()) == ((15 * dither) // 16 < 128), dither
        assert bool(M.ordered(white, dither).all()) == (255 + (-15 * dither) // 16 >= 128), dither
        assert ((15 * dither) // 16 < 128) == (dither <= 136) and (255 + (-15 * dither) // 16 >= 128) == (dither <= 135)


def test_luma_and_dither_offsets():
    assert M.luma(np.array([0, 0, 0])) == 0 and M.luma(np.array([255, 255, 255])) == 255
    assert M.luma(np.array([255, 0, 0])) == (77 * 255 + 128) >> 8
    # floor towards minus infinity: (2 * 0 - 15) * 32 / 16 = -30 exactly; amplitude 1: -15 / 16 -> -1, 15 / 16 -> 0
    Y = np.full((1, 192, 8), 128, np.int64)
    assert M.ordered(Y, 0).all()
    d1 = M.ordered(Y, 1)[0, :4, :4]
    assert np.array_equal(d1, (2 * M.BAYER - 15 >= 0).astype(np.uint8))


@pytest.mark.parametrize("mode", MODES)
def test_wavefront_diffusion_equals_the_raster_definition(mode):
    W = M.width(mode)
    rgb = np.concatenate([M.structured_frames(mode, 2), M.noise_frames(mode, 1), M.corner_frames(mode)[5:8]])
    Y = M.luma(rgb)
    assert Y.shape == (6, 192, W)
    assert np.array_equal(M.diffuse(Y), M.diffuse_raster(Y))


def _block_error(Y, d):
    """mean over blocks (28 dots x 8 rows) of |mean luminance shown - mean luminance asked for|, lit dots taken as 255"""
    H, W = Y.shape
    shown = (255.0 * d).reshape(H // 8, 8, W // 28, 28).mean(axis=(1, 3))
    asked = Y.astype(np.float64).reshape(H // 8, 8, W // 28, 28).mean(axis=(1, 3))
    return float(np.abs(shown - asked).mean())


@pytest.mark.parametrize("mode", MODES)
def test_dither_quality_order(mode):
    W = M.width(mode)
    y, x = np.mgrid[0:192, 0:W]
    ramp = x * 255 // (W - 1)
    vignette = np.clip(255 - ((x - W / 2) ** 2 / (W / 2) ** 2 + (y - 96) ** 2 / 96 ** 2) * 160, 0, 255).astype(np.int64)
    for name, g in (("ramp", ramp), ("vignette", vignette)):
        rgb = np.broadcast_to(g.astype(np.uint8)[None, ..., None], (1, 192, W, 3))
        Y = M.luma(rgb)[0]
        err = {d: _block_error(Y, M.dots(rgb, d)[0]) for d in (0, 32, M.DITHER_DIFFUSION)}
        print(name, mode, err)
        assert err[M.DITHER_DIFFUSION] < err[32] < err[0], (name, err)


@pytest.mark.parametrize("mode", MODES)
def test_oracle_table_builder_takes_dm_mono(O, mode):
    t = O.build_table(mode, M.dm_mono(), symmetric=True)
    assert t.shape == (O.num_offsets(mode), 1 << (2 * O.masked_bits(mode)))
    assert int(t.max()) <= 2047 and int(t.max()) <= 96 * O.masked_dots(mode)
    assert int(t.max()) > 0
