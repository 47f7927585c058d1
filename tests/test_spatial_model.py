"""CPU: section f16 of include/iivision.h as tests/spatial_model.py restates it, held to the consequences the section states; the two
table builders of frame_grabber.py; and the entry point's host side: the symbol, its place in the binding, and every refusal, which
the library decides before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import spatial_cases as SC
import spatial_model as M


def _noise(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def _random_taps(rng):
    cuts = np.sort(rng.integers(0, 257, 4))
    return tuple(int(v) for v in np.diff(np.concatenate([[0], cuts, [256]])))


# ---- the consequences of the rule ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", range(len(SC.TAP_PAIRS)))
def test_zero_gain_is_the_identity(pair):
    x = _noise(1, (2, 9, 12, 3))
    assert np.array_equal(M.filter_frames(x, *SC.TAP_PAIRS[pair], SC.GAINS["zero"]), x)


@pytest.mark.parametrize("gain", sorted(SC.GAINS))
def test_identity_taps_are_the_identity_whatever_the_gain(gain):
    x = _noise(2, (7, 8, 3))
    assert np.array_equal(M.blur(x, SC.IDENTITY_TAPS, SC.IDENTITY_TAPS), x)          # 65536 p + 32768 >> 16
    assert np.array_equal(M.filter_frames(x, SC.IDENTITY_TAPS, SC.IDENTITY_TAPS, SC.GAINS[gain]), x)


@pytest.mark.parametrize("pair", range(1, len(SC.TAP_PAIRS)))
def test_gain_minus_256_is_the_plain_blur(pair):
    x = _noise(3, (11, 16, 3))
    B = M.blur(x, *SC.TAP_PAIRS[pair])
    assert B.min() >= 0 and B.max() <= 255 and (B != x).any()
    assert np.array_equal(M.filter_frames(x, *SC.TAP_PAIRS[pair], SC.GAINS["blur"]), B)


@pytest.mark.parametrize("value", (0, 1, 137, 254, 255))
def test_a_constant_frame_is_a_fixed_point(value):
    x = np.full((6, 8, 3), value, np.uint8)
    x[..., 1] = 255 - value
    for pair in SC.TAP_PAIRS:
        for gain in SC.GAINS.values():
            assert np.array_equal(M.filter_frames(x, *pair, gain), x)


def test_separable_equals_direct():
    rng = np.random.default_rng(4)
    for shape in ((1, 4, 3), (2, 8, 3), (5, 4, 3), (3, 19, 24, 3)):
        x = _noise(rng.integers(1 << 30), shape)
        for pair in SC.TAP_PAIRS + tuple((_random_taps(rng), _random_taps(rng)) for _ in range(6)):
            assert np.array_equal(M.blur(x, *pair), M.blur_separable(x, *pair)), (shape, pair)
    # the extremes: h reaches 65280 and B 255 without a carry
    assert M.blur_separable(np.full((3, 4, 3), 255, np.uint8), SC.ASYMMETRIC_TAPS, SC.BINOMIAL_TAPS).max() == 255


def test_tap_order_and_axis_matter():
    x = _noise(5, (9, 12, 3))
    a, b = SC.ASYMMETRIC_TAPS, SC.BINOMIAL_TAPS
    base = M.filter_frames(x, a, b, SC.GAINS["blur"])
    assert (M.filter_frames(x, a[::-1], b, SC.GAINS["blur"]) != base).any()
    assert (M.filter_frames(x, b, a, SC.GAINS["blur"]) != base).any()
    # an impulse shows the orientation: tap k weighs the pixel at x + k - 2, so the impulse's image is the taps reversed
    imp = np.zeros((1, 12, 3), np.uint8)
    imp[0, 6] = 255
    got = M.blur(imp, a, SC.IDENTITY_TAPS)[0, 4:9, 0]
    assert got.tolist() == [(t * 255 * 256 + 32768) >> 16 for t in a[::-1]]


def test_edges_replicate():
    """a frame whose columns are 0 | 255: the blur at the left edge sees only zeros, at the right only 255s; a one-row frame is its
    own upper and lower neighbour"""
    x = np.zeros((1, 8, 3), np.uint8)
    x[:, 4:] = 255
    B = M.blur(x, SC.BINOMIAL_TAPS, SC.ASYMMETRIC_TAPS)
    assert (B[0, :2] == 0).all() and (B[0, 6:] == 255).all()
    assert np.array_equal(B, M.blur(x, SC.BINOMIAL_TAPS, SC.IDENTITY_TAPS))


# ---- the table builders ---------------------------------------------------------------------------------------------------------------

def test_filter_taps():
    import frame_grabber
    assert frame_grabber.BINOMIAL_TAPS == SC.BINOMIAL_TAPS == (16, 64, 96, 64, 16)
    assert frame_grabber.filter_taps(0) == SC.IDENTITY_TAPS
    for sigma in (0.1, 0.3, 0.5, 0.8, 1.0, 1.1, 1.5, 2.0, 5.0, 100.0):
        t = frame_grabber.filter_taps(sigma)
        assert len(t) == 5 and sum(t) == 256 and min(t) >= 0 and max(t) <= 256, (sigma, t)
        assert t[0] == t[4] and t[1] == t[3] and t[0] <= t[1] <= t[2], (sigma, t)
        w = np.exp(-np.arange(-2, 3) ** 2 / (2.0 * sigma * sigma))
        assert t[0] == int(np.floor(256 * w[0] / w.sum() + 0.5)) and t[1] == int(np.floor(256 * w[1] / w.sum() + 0.5))
    assert frame_grabber.filter_taps(0.1) == SC.IDENTITY_TAPS and frame_grabber.filter_taps(100.0) == (51, 51, 52, 51, 51)
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            frame_grabber.filter_taps(bad)


@pytest.mark.parametrize("lo,hi", [(0, 0), (0, 1), (4, 12), (8, 8), (0, 255), (255, 255), (100, 101)])
def test_denoise_gain(lo, hi):
    import frame_grabber
    g = frame_grabber.filter_gain(denoise=(lo, hi))
    assert g.dtype == np.int16 and g.shape == (256,) and np.array_equal(g, SC.gain_table(denoise=(lo, hi)))
    assert (np.diff(g.astype(int)) >= 0).all()                                    # monotone over the whole branch
    assert (g[:lo + 1] == -256).all() and (g[hi + 1:] == 0).all()                 # the ends are lo and hi
    between = g[lo + 1:hi + 1].astype(int)
    assert len(between) == hi - lo and (between > -256).all() and (between < 0).all()
    for m in range(lo + 1, hi + 1):
        assert g[m] == -256 + (256 * (m - lo)) // (hi - lo + 1)


def test_sharpen_gain_and_both():
    import frame_grabber
    assert not frame_grabber.filter_gain().any()
    assert not frame_grabber.filter_gain(denoise=(0, 0))[1:].any()               # all zero beyond m = 0
    for amount, threshold in ((0, 0), (256, 0), (384, 16), (1024, 254), (77, 255)):
        g = frame_grabber.filter_gain(sharpen=(amount, threshold))
        assert not g[:threshold + 1].any() and (g[threshold + 1:] == amount).all()
        assert (np.diff(g.astype(int)) >= 0).all()
    g = frame_grabber.filter_gain(denoise=(4, 12), sharpen=(384, 16))
    assert np.array_equal(g, SC.GAINS["both"])
    assert (g[:5] == -256).all() and (np.diff(g[:13].astype(int)) >= 0).all() and not g[13:17].any() and (g[17:] == 384).all()
    g = frame_grabber.filter_gain(denoise=(4, 12), sharpen=(384, 12))            # threshold == hi: the branches meet
    assert g[12] < 0 and g[13] == 384
    for kw in (dict(denoise=(5, 4)), dict(denoise=(-1, 4)), dict(denoise=(0, 256)), dict(denoise=(1.5, 3)), dict(denoise=(1,)),
               dict(sharpen=(1025, 0)), dict(sharpen=(-1, 0)), dict(sharpen=(256, 256)), dict(sharpen="ab"),
               dict(denoise=(4, 12), sharpen=(384, 11))):
        with pytest.raises(ValueError):
            frame_grabber.filter_gain(**kw)


def test_spatial_holds_the_tables():
    import frame_grabber
    s = frame_grabber.Spatial(denoise=(4, 12), sharpen=(384, 16))
    assert s.taps_x == s.taps_y == SC.BINOMIAL_TAPS and np.array_equal(s.gain, SC.GAINS["both"])
    s = frame_grabber.Spatial(blur=(1.0, 0))
    assert s.taps_x == frame_grabber.filter_taps(1.0) and s.taps_y == SC.IDENTITY_TAPS and not s.gain.any()
    for kw in (dict(blur=1.0), dict(blur=(1, 2, 3)), dict(blur=(-1, 1)), dict(denoise=(9, 3))):
        with pytest.raises(ValueError):
            frame_grabber.Spatial(**kw)


# ---- what the two uses do ------------------------------------------------------------------------------------------------------------

def test_sharpen_grows_the_contrast_at_a_step_and_clamps():
    import frame_grabber
    gain = frame_grabber.filter_gain(sharpen=(256, 0))
    x = np.zeros((6, 16, 3), np.uint8)
    x[:, 8:] = 255
    y = M.filter_frames(x, SC.BINOMIAL_TAPS, SC.BINOMIAL_TAPS, gain)
    B = M.blur(x, SC.BINOMIAL_TAPS, SC.BINOMIAL_TAPS)
    assert 0 < B[0, 7, 0] < B[0, 8, 0] < 255                                      # the blur softens the edge ...
    assert 2 * 0 - int(B[0, 7, 0]) < 0 and 2 * 255 - int(B[0, 8, 0]) > 255        # ... so p + (p - B) overshoots on both sides
    assert np.array_equal(y, x)                                                   # and clamps at 0 and 255: a full step stays
    # a softer step inside the range: the contrast next to the edge grows, the overshoot is there and unclamped
    x = np.full((6, 16, 3), 64, np.uint8)
    x[:, 8:] = 192
    y = M.filter_frames(x, SC.BINOMIAL_TAPS, SC.BINOMIAL_TAPS, gain).astype(int)
    assert y[0, 8, 0] - y[0, 7, 0] > 192 - 64 and y[0, 7, 0] < 64 and y[0, 8, 0] > 192
    assert (y[:, :5] == 64).all() and (y[:, 11:] == 192).all()                    # away from the edge nothing moves
    # with the gain at its largest the same step clamps at both ends
    y = M.filter_frames(np.where(x == 64, 8, 247).astype(np.uint8), SC.BINOMIAL_TAPS, SC.BINOMIAL_TAPS, SC.GAINS["most"])
    assert y[0, 7, 0] == 0 and y[0, 8, 0] == 255


def test_denoise_takes_flat_noise_to_the_blur():
    import frame_grabber
    rng = np.random.default_rng(1603)
    x = (128 + rng.integers(-3, 4, (2, 48, 64, 3))).astype(np.uint8)
    B = M.blur(x, SC.BINOMIAL_TAPS, SC.BINOMIAL_TAPS)
    m = np.abs(x.astype(int) - B).max()
    assert m <= 8, m
    y = M.filter_frames(x, SC.BINOMIAL_TAPS, SC.BINOMIAL_TAPS, frame_grabber.filter_gain(denoise=(8, 8)))
    assert np.array_equal(y, B)
    assert y.astype(float).std() < x.astype(float).std()
    # an edge far above hi is left alone where the noise is not
    e = x.copy()
    e[:, :, 32:] += 100
    y = M.filter_frames(e, SC.BINOMIAL_TAPS, SC.BINOMIAL_TAPS, frame_grabber.filter_gain(denoise=(8, 8)))
    assert np.array_equal(y[:, :, 31:33], e[:, :, 31:33]) and (y[:, :, :28] != e[:, :, :28]).any()


def test_the_gpu_grid_meets_every_branch():
    """the inputs of tests/test_gpu_spatial.py, on the model: under the denoise-and-sharpen table they meet all three branches, the
    largest gain clamps at both ends, and every (H, W) of the grid has its impulses on both sides of every seam"""
    for H, W in ((SC.T_H + 1, SC.T_W + 4), (5, 280)):
        x, B = SC.block(H, W), SC.blurred(H, W, 1)
        m = np.abs(x.astype(int) - B).max(axis=-1)
        g = SC.GAINS["both"].astype(int)[m]
        assert (g < 0).any() and (g == 0).any() and (g > 0).any()
        y = SC.want(H, W, 1, "most")
        assert ((y == 0) & (x != 0)).any() and ((y == 255) & (x != 255)).any()
    pts = SC.impulse_points(2 * SC.T_H + 3, SC.T_W + 4)
    for p in ((SC.T_H - 1, (SC.T_W + 4) // 2), (SC.T_H, (SC.T_W + 4) // 2), (2 * SC.T_H - 1, (SC.T_W + 4) // 2),
              (SC.T_H + 1, SC.T_W - 1), (SC.T_H + 1, SC.T_W), (SC.T_H - 1, SC.T_W - 1), (2 * SC.T_H, SC.T_W), (0, 0)):
        assert p in pts, p
    assert len(SC.impulse_points(1, 4)) == 3 and SC.block(1, 4).shape == (3, 3, 1, 4, 3)
    for H in SC.HEIGHTS:
        for W in SC.WIDTHS:
            assert int((SC.block(H, W)[1:] == 255).all(axis=-1).sum()) == len(SC.impulse_points(H, W))


# ---- the entry point's host side -----------------------------------------------------------------------------------------------------

def test_the_entry_point_is_declared_and_exported(native):
    assert "iiv_filter_frames" in native.SYMBOLS
    f = native.lib().iiv_filter_frames
    assert f.restype is C.c_int and len(f.argtypes) == 14 and f.argtypes[2] is C.c_int and f.argtypes[5] is C.c_size_t


def _arr(values, ctype):
    return (ctype * len(values))(*values)


def test_refusals_need_no_device(native):
    """every refusal of the header, with device pointers that are never followed: the library decides before anything is launched"""
    L = native.lib()
    base = 1 << 20
    good_x, good_y = _arr(SC.ASYMMETRIC_TAPS, C.c_uint16), _arr(SC.BINOMIAL_TAPS, C.c_uint16)
    good_g = _arr([int(v) for v in SC.GAINS["both"]], C.c_int16)

    def taps(*v):
        return _arr(v, C.c_uint16)

    def gain(at, value):
        g = [0] * 256
        g[at] = value
        return _arr(g, C.c_int16)

    def call(c=2, n=3, h=2, w=4, src=base, scs=96, sfs=24, out=base + 4096, ocs=96, ofs=24, tx=good_x, ty=good_y, g=good_g):
        return L.iiv_filter_frames(c, n, h, w, C.c_void_p(src), scs, sfs, C.c_void_p(out), ocs, ofs, tx, ty, g, None)
    assert call(c=0) == 0                                                      # (the good call's arguments pass every check)
    refused = [call(c=-1), call(n=-1), call(h=0), call(w=0), call(h=-2, w=4), call(h=1, w=6, sfs=24), call(h=3, w=3, sfs=32),
               call(h=4097, w=4096, sfs=1 << 26, ofs=1 << 26, scs=1 << 28, ocs=1 << 28),                    # pixels above 2^24
               call(src=base + 2), call(out=base + 4097), call(scs=98), call(sfs=26), call(ocs=94), call(ofs=30),
               call(sfs=20), call(ofs=20),
               call(h=-1, w=-8), call(h=4100, w=4, sfs=49200, ofs=49200, scs=1 << 18, ocs=1 << 18),          # height outside 1..4096
               call(h=1, w=4100, sfs=12300, ofs=12300, scs=1 << 16, ocs=1 << 16), call(h=2, w=2, sfs=12), call(h=2, w=6, sfs=36, ofs=36, scs=144, ocs=144),
               call(tx=None), call(ty=None), call(g=None),
               call(tx=taps(0, 0, 257, 0, 0)), call(ty=taps(0, 0, 0, 0, 65535)), call(tx=taps(16, 64, 96, 64, 15)),
               call(ty=taps(16, 64, 96, 64, 17)), call(tx=taps(0, 0, 0, 0, 0)), call(ty=taps(256, 256, 256, 256, 256)),
               call(g=gain(0, -257)), call(g=gain(255, 1025)), call(g=gain(100, 32767)), call(g=gain(17, -32768)),
               call(out=base), call(src=0), call(out=0), call(src=0, out=0)]
    assert refused == [native.ERR_INVALID] * len(refused)
    assert b"iiv_filter_frames" in L.iiv_last_error()
    # the extremes that are allowed, and no work: success, nothing touched (the pointers are not even looked at)
    assert call(c=0, g=gain(0, -256)) == 0 and call(n=0, g=gain(255, 1024)) == 0 and call(c=0, tx=taps(256, 0, 0, 0, 0)) == 0
    assert call(c=0, h=4096, w=4096, sfs=1 << 26, ofs=1 << 26, scs=1 << 28, ocs=1 << 28) == 0
    assert call(c=0) == 0 and call(n=0) == 0 and call(c=0, src=0, out=0) == 0
    # in the header's order: what the shared front refuses comes before the stage's own
    assert call(c=-1, h=5000) == native.ERR_INVALID and b"n_clips" in L.iiv_last_error()
    assert call(h=5000, w=4, sfs=60000, ofs=60000, scs=1 << 18, ocs=1 << 18, tx=None) == native.ERR_INVALID and b"height" in L.iiv_last_error()
    assert call(tx=taps(0, 0, 255, 0, 0), out=base) == native.ERR_INVALID and b"sum" in L.iiv_last_error()
    assert call(g=gain(3, 2000), out=base) == native.ERR_INVALID and b"gain" in L.iiv_last_error()
    assert call(out=base, src=base) == native.ERR_INVALID and b"d_out == d_src" in L.iiv_last_error()


def test_the_binding_refuses_bad_tables():
    """filter_tables decides before any device is asked for"""
    import _iiv_native as native
    tx, ty, g = native.filter_tables(SC.ASYMMETRIC_TAPS, list(SC.BINOMIAL_TAPS), SC.GAINS["random"])
    assert tx.dtype == np.uint16 and tx.tolist() == list(SC.ASYMMETRIC_TAPS) and ty.tolist() == list(SC.BINOMIAL_TAPS)
    assert g.dtype == np.int16 and np.array_equal(g, SC.GAINS["random"]) and g.flags.c_contiguous
    assert native.filter_tables((256, 0, 0, 0, 0), (0, 0, 0, 0, 256), np.full(256, 1024))[2].max() == 1024
    good = (SC.BINOMIAL_TAPS, SC.BINOMIAL_TAPS, SC.GAINS["zero"])
    for at, bad in ((0, (16, 64, 96, 64)), (1, (16, 64, 97, 64, 16)), (0, (0, 0, 257, 0, -1)), (1, (0.5, 0.5, 255, 0, 0)), (0, None),
                    (1, (300, 0, 0, 0, -44)), (2, np.zeros(255, np.int16)), (2, np.full(256, -257)), (2, np.full(256, 1025)),
                    (2, np.zeros(256, np.float32)), (2, np.full(256, 70000))):
        args = list(good)
        args[at] = bad
        with pytest.raises(ValueError):
            native.filter_tables(*args)
