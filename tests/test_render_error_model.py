"""CPU: tests/render_error_model.py (the numpy restatement of include/iivision.h "f8: screen error") against sums derived by
hand, and screen.psnr against the formulas written out here."""
import math
import os
import sys

import numpy as np
import pytest

import render_error_model as E
import render_model as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ii-vision_amd", "transcoder"))

PAL = ((np.arange(48) * 37 + 11) % 256).astype(np.uint8).reshape(16, 3)
BLACK = np.zeros((16, 3), np.uint8)


@pytest.mark.parametrize("width", [280, 560])
@pytest.mark.parametrize("mode", [R.HGR, R.DHGR])
def test_black_screen_against_a_constant_reference(mode, width):
    a, b, c = 3, 100, 255
    ref = np.empty((2, 192, width, 3), np.uint8)
    ref[:] = (a, b, c)
    zero = np.zeros((2, 32, 256), np.uint8)
    got = E.render_error(mode, zero, zero, BLACK, ref)
    assert got.dtype == np.uint64 and got.shape == (2, 3, 3)
    for ch, v in enumerate((a, b, c)):
        assert got[:, 0, ch].tolist() == [107520 * v * v] * 2
        assert got[:, 1, ch].tolist() == [26880 * (4 * v) ** 2] * 2
        assert got[:, 2, ch].tolist() == [6720 * (16 * v) ** 2] * 2
    assert int(got[0, 0, 2]) > 2 ** 32        # 255 everywhere: past 32 bits at every level


@pytest.mark.parametrize("mode", [R.HGR, R.DHGR])
def test_reference_equal_to_the_rendering_gives_zero(mode):
    rng = np.random.default_rng(5 + mode)
    main, aux = rng.integers(0, 256, (2, 32, 256), dtype=np.uint8), rng.integers(0, 256, (2, 32, 256), dtype=np.uint8)
    shot = R.render_rgb(mode, main, aux, PAL)
    assert not E.render_error(mode, main, aux, PAL, shot).any()
    # one byte of one dot off by 7: its square at every level (the only nonzero difference of its quad and unit)
    shot[1, 100, 333, 1] ^= 7
    want = np.zeros((2, 3, 3), np.uint64)
    d = int(shot[1, 100, 333, 1]) - int(shot[1, 100, 333, 1] ^ 7)
    want[1, :, 1] = d * d
    assert (E.render_error(mode, main, aux, PAL, shot) == want).all()


def test_width_280_against_aligned_repeating_quads_by_a_direct_loop():
    """DHGR rows of one aligned repeating quad each (row y: quad y & 15), a random 280-wide reference: the sums by a loop over
    the dots, with the colour of dot x written out (value P from dot 3 on; the window is still filling before)."""
    rng = np.random.default_rng(11)
    main, aux = np.zeros((1, 32, 256), np.uint8), np.zeros((1, 32, 256), np.uint8)
    fm, fa = main.reshape(1, 8192), aux.reshape(1, 8192)
    for y in range(192):
        a, m = R.dhgr_quad_row(y & 15)
        fa[0, R.ROW_OFFSET[y]:R.ROW_OFFSET[y] + 40], fm[0, R.ROW_OFFSET[y]:R.ROW_OFFSET[y] + 40] = a, m
    ref = rng.integers(0, 256, (1, 192, 280, 3), dtype=np.uint8)
    want = [[0] * 3 for _ in range(3)]
    for y in range(192):
        P = y & 15
        for ch in range(3):
            quad = unit = 0
            for x in range(560):
                if x >= 3:
                    value = P
                else:       # dots 0 .. x of the quad in the window's top bits, rotated by (x + 1) & 3
                    w = sum(((P >> k) & 1) << (3 - x + k) for k in range(x + 1))
                    value = R.rol4(w, (x + 1) & 3)
                d = int(PAL[value, ch]) - int(ref[0, y, x // 2, ch])
                want[0][ch] += d * d
                quad += d
                unit += d
                if x % 4 == 3:
                    want[1][ch] += quad * quad
                    quad = 0
                if x % 16 == 15:
                    want[2][ch] += unit * unit
                    unit = 0
    got = E.render_error(R.DHGR, main, aux, PAL, ref)
    assert got[0].tolist() == want


def test_psnr_formulas():
    import screen
    a = 16
    ref = np.full((1, 192, 560, 3), a, np.uint8)
    ref[..., 1] = 0
    ref[..., 2] = 255
    zero = np.zeros((1, 32, 256), np.uint8)
    sums = E.render_error(R.DHGR, zero, zero, BLACK, ref)
    for level, (cells, k) in enumerate(((107520, 1), (26880, 4), (6720, 16))):
        per, overall = screen.psnr(sums, level)
        assert per.dtype == np.float64 and per.shape == (1, 3) and overall.shape == (1,)
        # a constant difference a: sum = cells (k a)^2, so the PSNR is 20 log10(255 / a) at every level
        assert per[0, 0] == pytest.approx(20 * math.log10(255 / a), abs=1e-12)
        assert per[0, 0] == pytest.approx(10 * math.log10(255 ** 2 * cells * k * k / int(sums[0, level, 0])), abs=1e-12)
        assert per[0, 1] == math.inf                       # a zero sum
        assert per[0, 2] == pytest.approx(0.0, abs=1e-12)  # as wrong as can be
        total = sum(int(v) for v in sums[0, level])
        assert overall[0] == pytest.approx(10 * math.log10(255 ** 2 * 3 * cells * k * k / total), abs=1e-12)
        mper, mall = E.psnr(sums, level)
        assert (mper == per).all() and (mall == overall).all()
    per, overall = screen.psnr(np.zeros((3, 3), np.uint64))            # level 0 by default; all zero: inf overall too
    assert (per == math.inf).all() and overall == math.inf
