"""CPU: the resize's contract (include/iivision.h: iiv_resize_coeffs / iiv_resize_frames) -- the tests'
numpy model (tests/resize_model.py) equals the installed Pillow's Image.resize(..., LANCZOS) byte for byte, and the
library's host-side coefficient tables equal the model's.  No GPU."""
import numpy as np
import pytest

import resize_model as M


def _frames(h, w, n, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)


FIXED, RANDOM = M.sizes()


@pytest.mark.parametrize("h,w,H,W", FIXED)
def test_model_equals_pillow_fixed(h, w, H, W):
    pytest.importorskip("PIL")
    a = _frames(h, w, 1 if h * w > 100000 else 2, h * 7 + w)
    assert np.array_equal(M.resize(a, (H, W)), M.pillow_resize(a, (H, W)))


def test_model_equals_pillow_random_pairs():
    pytest.importorskip("PIL")
    for i, (h, w, H, W) in enumerate(RANDOM):
        a = _frames(h, w, 1, i)
        assert np.array_equal(M.resize(a, (H, W)), M.pillow_resize(a, (H, W))), (h, w, H, W)


def test_pass_order_boundary():
    """h > 100 w: the vertical pass first, else the horizontal one; both sides of the boundary differ in at least one
    of these seeded frames, so the order is pinned, not only stated"""
    assert M.vertical_first(401, 4) and not M.vertical_first(400, 4)
    pytest.importorskip("PIL")
    for h, w in ((401, 4), (301, 3)):
        a = _frames(h, w, 1, 11)
        H, W = 17, 9
        h_first = M._pass(M._pass(a, 2, W), 1, H)
        v_first = M._pass(M._pass(a, 1, H), 2, W)
        pil = M.pillow_resize(a, (H, W))
        assert np.array_equal(pil, v_first)
        assert not np.array_equal(h_first, v_first)


PAIRS = [(640, 280), (480, 192), (1920, 280), (1080, 192), (1280, 280), (720, 192), (53, 280), (37, 192), (1, 280),
         (2000, 1), (8192, 1024), (8192, 1), (1, 1), (280, 280), (192, 192), (3, 1000), (999, 997), (4096, 7)]


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_native_coeffs_equal_model(native, n_in, n_out):
    ks, bounds, k = M.coeffs(n_in, n_out)
    nb, nk = native.resize_coeffs(n_in, n_out)
    assert nk.shape == (n_out, ks)
    assert np.array_equal(nb, bounds)
    assert np.array_equal(nk, k)


def test_native_coeffs_random_pairs(native):
    rng = np.random.RandomState(99)
    for _ in range(60):
        n_in, n_out = int(rng.randint(1, 8193)), int(rng.randint(1, 1025))
        _, bounds, k = M.coeffs(n_in, n_out)
        nb, nk = native.resize_coeffs(n_in, n_out)
        assert np.array_equal(nb, bounds) and np.array_equal(nk, k), (n_in, n_out)


def test_same_size_table_is_the_identity(native):
    """(h, w) == (H, W) is a copy in Pillow; the library runs it as a pass with the in == out table, which is one unit tap"""
    for n in (1, 2, 7, 192, 280, 1024):
        bounds, k = native.resize_coeffs(n, n)
        rows = np.arange(n)
        taps = rows - bounds[:, 0]
        assert (k[rows, taps] == 1 << M.PRECISION_BITS).all()
        assert (np.abs(k).sum(axis=1) == 1 << M.PRECISION_BITS).all()


def test_fixed_point_sum_cannot_overflow(native):
    for n_in, n_out in PAIRS:
        _, k = native.resize_coeffs(n_in, n_out)
        assert 255 * int(np.abs(k.astype(np.int64)).sum(axis=1).max()) + (1 << 21) < 2 ** 31


def test_host_entry_point_refuses_out_of_domain(native):
    import ctypes as C
    L = native.lib()
    ks = C.c_int(0)
    for n_in, n_out in ((0, 1), (1, 0), (8193, 1), (1, 1025), (-5, 10)):
        assert L.iiv_resize_coeffs(n_in, n_out, C.byref(ks), None, None) == native.ERR_INVALID
        with pytest.raises(native.IIVError):
            native.resize_coeffs(n_in, n_out)
    assert L.iiv_resize_coeffs(8192, 1024, None, None, None) == native.ERR_INVALID
    b = np.zeros((4, 2), np.int32)
    assert L.iiv_resize_coeffs(10, 4, C.byref(ks), native.hptr(b), None) == native.ERR_INVALID
    assert L.iiv_resize_coeffs(8192, 1024, C.byref(ks), None, None) == native.OK and ks.value == 49


def test_frames_entry_point_refuses_out_of_domain_before_launch(native):
    """refusals need no device: nothing is launched (the pointers are never touched)"""
    L = native.lib()
    p = native.C.c_void_p(16)
    for args in ((1, 0, 10, 30, 30, 192, 280), (1, 10, 8193, 30, 30 * 8193, 192, 280), (1, 10, 10, 300, 30, 1025, 280),
                 (1, 10, 10, 300, 30, 192, 0), (-1, 10, 10, 300, 30, 192, 280),
                 (2, 10, 10, 299, 30, 192, 280),        # frames overlap
                 (1, 10, 10, 300, 29, 192, 280)):       # rows overlap
        n, h, w, fs, rs, H, W = args
        assert L.iiv_resize_frames(n, h, w, p, fs, rs, H, W, p, None) == native.ERR_INVALID, args
    assert L.iiv_resize_frames(0, 480, 640, None, 0, 0, 192, 280, None, None) == native.OK
    assert L.iiv_resize_frames(1, 480, 640, None, 0, 1920, 192, 280, p, None) == native.ERR_INVALID
