"""GPU: rgb_to_lab and delta_e_cie2000 of csrc/iiv_tables.hip, through iiv_cie2000_matrix and iiv_delta_e_cie2000, against
tests/colour_model.py (50 digits) on the committed case set of tests/colour_cases.py.  Every float comparison is absolute, at
colour_model.T = 8 E_HOST = 2.32e-11 (E_HOST: the host oracle's own distance from the model on the same cases, measured in
tests/test_colour_model.py, which also checks that no case sits where a correct libm could land on the other side of an int()
or of a discontinuity of the formula).

Measured on an MI355X: the largest |device - model| is 6.84e-12 (the IIGS palette; NTSC 1.95e-12, every palette without a
grey against a saturated colour below 1.5e-13, the Lab pairs 1.4e-13 at most, the colour stage of stage_fuzz alike).
"""
import numpy as np
import pytest

import colour_cases as CC
import colour_model as M

pytestmark = pytest.mark.gpu
T = M.T
SENTINEL_F, SENTINEL_I = -12345.678, -1234567


def _report(capsys, what, err):
    with capsys.disabled():
        print("\n%s: largest |device - model| %.3g (T = %.3g)" % (what, err, T))


def _matrix(native, pal, want_f=True, want_i=True):
    """one raw call: -> (rc, the float array, the int array), an array that is not handed over keeps its sentinel fill"""
    rgb = np.ascontiguousarray(pal, dtype=np.uint8).reshape(48)
    f, i = np.full((16, 16), SENTINEL_F), np.full((16, 16), SENTINEL_I, dtype=np.int32)
    rc = native.lib().iiv_cie2000_matrix(native.hptr(rgb), native.hptr(f) if want_f else None,
                                         native.hptr(i) if want_i else None, native.stream_ptr())
    return rc, f, i


@pytest.mark.parametrize("name", CC.PALETTE_NAMES)
def test_matrix_against_the_model(native, name, capsys):
    pal = CC.palettes()[name]
    want_f, want_i = CC.model_matrix(name)
    rc, f, i = _matrix(native, pal)
    native.check(rc)
    assert not np.isnan(f).any()
    err = np.abs(f - want_f)
    _report(capsys, "cie2000_matrix %s" % name, err.max())
    assert err.max() <= T, (divmod(int(err.argmax()), 16), err.max())
    assert np.array_equal(i, want_i), np.argwhere(i != want_i)
    same = (pal[:, None, :] == pal[None, :, :]).all(axis=2)                     # the diagonal and every repeated colour
    assert same.diagonal().all() and not f[same].any() and not np.signbit(f[same]).any()
    assert (f[~same] > 0).all()
    assert np.abs(f - f.T).max() <= T
    # either output alone: the same values, and nothing into the array that was not handed over
    rc, f_none, i_only = _matrix(native, pal, want_f=False)
    native.check(rc)
    assert np.array_equal(i_only, i) and (f_none == SENTINEL_F).all()
    rc, f_only, i_none = _matrix(native, pal, want_i=False)
    native.check(rc)
    assert np.array_equal(f_only, f) and not np.signbit(f_only[same]).any() and (i_none == SENTINEL_I).all()


def test_matrix_refuses_a_null_palette(native):
    rgb = np.zeros(48, dtype=np.uint8)
    f, i = np.full((16, 16), SENTINEL_F), np.full((16, 16), SENTINEL_I, dtype=np.int32)
    rc = native.lib().iiv_cie2000_matrix(None, native.hptr(f), native.hptr(i), native.stream_ptr())
    assert rc == native.ERR_INVALID and (f == SENTINEL_F).all() and (i == SENTINEL_I).all()
    native.check(native.lib().iiv_cie2000_matrix(native.hptr(rgb), native.hptr(f), native.hptr(i), native.stream_ptr()))   # and goes on working
    assert not f.any() and not i.any()


GUARD = 8


def _pairs(native, n, lab1, lab2, out="own"):
    """one raw call on n pairs, the output between GUARD sentinel doubles either side in one host buffer -> (rc, that buffer)"""
    a, b = (np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3) if v is not None else None for v in (lab1, lab2))
    buf = np.full(2 * GUARD + max(n, 0), SENTINEL_F)
    rc = native.lib().iiv_delta_e_cie2000(n, native.hptr(a) if a is not None else None, native.hptr(b) if b is not None else None,
                                          native.hptr(buf[GUARD:]) if out is not None else None, native.stream_ptr())
    return rc, buf


@pytest.mark.parametrize("n", CC.COUNTS)
def test_pairs_against_the_model(native, n, capsys):
    kinds, lab1, lab2 = CC.pool()
    idx = CC.subset(n)
    want = CC.model_pool()[idx]
    rc, buf = _pairs(native, n, lab1[idx], lab2[idx])
    native.check(rc)
    got = buf[GUARD:GUARD + n]
    assert (buf[:GUARD] == SENTINEL_F).all() and (buf[GUARD + n:] == SENTINEL_F).all()            # not a double outside out[0 .. n - 1]
    assert not np.isnan(got).any() and (got != SENTINEL_F).all()                                   # and every one inside written
    err = np.abs(got - want)
    _report(capsys, "delta_e_cie2000 n = %d" % n, err.max())
    worst = int(err.argmax())
    assert err.max() <= T, (int(idx[worst]), kinds[idx[worst]], lab1[idx[worst]], lab2[idx[worst]], got[worst], want[worst])
    identical = (lab1[idx] == lab2[idx]).all(axis=1)
    assert not got[identical].any() and not np.signbit(got[identical]).any()


def test_pairs_no_pairs_and_refusals(native):
    _, lab1, lab2 = CC.pool()
    a, b = lab1[:4], lab2[:4]
    rc, buf = _pairs(native, 0, a, b)
    assert rc == native.OK and (buf == SENTINEL_F).all()
    for n, x, y, out in ((-1, a, b, "own"), (-(1 << 31), a, b, "own"), (4, None, b, "own"), (4, a, None, "own"), (4, a, b, None)):
        rc, buf = _pairs(native, n, x, y, out)
        assert rc == native.ERR_INVALID and (buf == SENTINEL_F).all(), (n, x is None, y is None, out)
    rc, buf = _pairs(native, 4, a, b)                                                              # and goes on working
    native.check(rc)
    assert np.abs(buf[GUARD:GUARD + 4] - CC.model_pool()[:4]).max() <= T and (buf[GUARD + 4:] == SENTINEL_F).all()
