"""CPU: section f15 of include/iivision.h as tests/levels_model.py restates it, held to the properties the section states; the host
closed form iiv_levels_auto and the two Python table builders against the model; and the host side of the three entry points: the
symbols, their place in the binding, and every refusal, which the library decides before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import levels_cases as LC
import levels_model as M


def _auto(native, hist, lo, hi):
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    black, white = C.c_int(-7), C.c_int(-7)
    rc = native.lib().iiv_levels_auto(h.ctypes.data_as(C.c_void_p), lo, hi, C.byref(black), C.byref(white))
    return rc, (black.value, white.value)


PPMS = ((5000, 5000), (0, 0), (500000, 500000), (0, 500000), (500000, 0), (1, 1), (250000, 100000), (999, 123456))


def _histograms():
    rng = np.random.default_rng(1501)
    hs = {"empty": np.zeros(256, np.uint64)}
    for i in range(6):
        hs["random %d" % i] = rng.integers(0, min(10 ** (1 + 2 * i), 2 ** 35), 256).astype(np.uint64)   # (256 * 2^35 = 2^43)
    sparse = np.zeros(256, np.uint64)
    sparse[rng.integers(0, 256, 9)] = rng.integers(1, 1000, 9).astype(np.uint64)
    hs["sparse"] = sparse
    for v in (0, 1, 128, 254, 255):
        one = np.zeros(256, np.uint64)
        one[v] = 53760
        hs["one bin %d" % v] = one
    for v in (0, 100, 254):
        for counts in ((1, 1), (1000, 3), (3, 1000), (199, 1)):
            two = np.zeros(256, np.uint64)
            two[v], two[v + 1] = counts
            hs["two bins %d %s" % (v, counts)] = two
    ends = np.zeros(256, np.uint64)
    ends[0], ends[255] = 1, 1
    hs["ends"] = ends
    big = np.zeros(256, np.uint64)
    big[10], big[200] = 2 ** 42, 2 ** 42
    hs["2^43"] = big
    spread = np.full(256, 2 ** 35, np.uint64)
    hs["2^43 spread"] = spread
    return hs


def test_auto_equals_the_model(native):
    for name, h in _histograms().items():
        for lo, hi in PPMS:
            rc, got = _auto(native, h, lo, hi)
            assert rc == 0 and got == M.auto(h, lo, hi), (name, lo, hi, got, M.auto(h, lo, hi))
            assert native.levels_auto(h, lo, hi) == got
    assert int(_histograms()["2^43"].sum()) == 2 ** 43 == int(_histograms()["2^43 spread"].sum())
    assert native.levels_auto(np.zeros(256, np.int64)) == (0, 255)


def test_auto_properties(native):
    """what the definition promises: at most k pixels outside the points, and the points are occupied bins"""
    for name, h in _histograms().items():
        total = int(h.astype(object).sum())
        for lo, hi in PPMS:
            black, white = native.levels_auto(h, lo, hi)
            if (black, white) == (0, 255) and (total == 0 or M.auto(h, lo, hi) == (0, 255)):
                continue
            assert black < white and h[black] > 0 and h[white] > 0
            assert int(h[:black].astype(object).sum()) <= total * lo // 10 ** 6
            assert int(h[white + 1:].astype(object).sum()) <= total * hi // 10 ** 6
    # one bin, two adjacent bins at half and half, and an empty histogram are the identity range
    assert M.auto(_histograms()["one bin 128"]) == (0, 255) and M.auto(_histograms()["empty"]) == (0, 255)
    assert M.auto(_histograms()["two bins 100 (1, 1)"], 0, 0) == (100, 101)
    assert M.auto(_histograms()["two bins 100 (199, 1)"], 5000, 5000) == (0, 255)     # k = 1: the single pixel at 101 is cut off
    assert M.auto(_histograms()["ends"], 0, 0) == (0, 255) and M.auto(_histograms()["ends"], 500000, 500000) == (0, 255)


def test_auto_refusals(native):
    L = native.lib()
    h = np.zeros(256, np.uint64)
    h[3], h[77] = 2 ** 43, 1                      # 2^43 + 1
    assert _auto(native, h, 5000, 5000) == (native.ERR_INVALID, (-7, -7))
    assert b"iiv_levels_auto" in L.iiv_last_error()
    h[3] = 2 ** 43 - 1
    assert _auto(native, h, 5000, 5000)[0] == 0   # exactly 2^43
    wrap = np.full(256, 2 ** 56, np.uint64)       # the sum of these is 0 modulo 2^64
    assert _auto(native, wrap, 0, 0)[0] == native.ERR_INVALID
    ok = np.ones(256, np.uint64)
    assert _auto(native, ok, 500001, 0)[0] == native.ERR_INVALID and _auto(native, ok, 0, 500001)[0] == native.ERR_INVALID
    assert _auto(native, ok, 2 ** 32 - 1, 0)[0] == native.ERR_INVALID
    b, w = C.c_int(0), C.c_int(0)
    p = ok.ctypes.data_as(C.c_void_p)
    assert L.iiv_levels_auto(None, 0, 0, C.byref(b), C.byref(w)) == native.ERR_INVALID
    assert L.iiv_levels_auto(p, 0, 0, None, C.byref(w)) == native.ERR_INVALID
    assert L.iiv_levels_auto(p, 0, 0, C.byref(b), None) == native.ERR_INVALID
    for bad in (dict(lo_ppm=-1), dict(hi_ppm=500001), dict(lo_ppm=0.5)):
        with pytest.raises(ValueError):
            native.levels_auto(ok, **bad)
    for bad in (np.ones(255, np.int64), np.ones(256), -np.ones(256, np.int64), np.ones((2, 256), np.int64)):
        with pytest.raises(ValueError):
            native.levels_auto(bad)


# ---- the table builders ------------------------------------------------------------------------------------------------------------

def test_linear_table_fixed_points_for_every_pair():
    import frame_grabber
    assert np.array_equal(frame_grabber.levels_lut(), M.IDENTITY_LUT) and np.array_equal(M.linear_lut(0, 255), M.IDENTITY_LUT)
    for black in range(255):
        for white in range(black + 1, 256):
            lut = frame_grabber.levels_lut(black, white)
            assert lut.dtype == np.uint8 and lut.shape == (256,)
            assert lut[black] == 0 and lut[white] == 255 and (lut[:black] == 0).all() and (lut[white:] == 255).all(), (black, white)
            if (black * 7 + white) % 16 == 0 or white - black < 3:     # the model's Python-integer table on a sixteenth of the pairs
                assert np.array_equal(lut, M.linear_lut(black, white)), (black, white)
            assert (np.diff(lut.astype(int)) >= 0).all()


def test_neutral_curve_is_skipped(monkeypatch):
    """at gamma = 1, brightness = 0, contrast = 1 the float curve is not evaluated at all: with np.floor disabled the table still
    comes out; away from neutral the same call needs it"""
    import frame_grabber

    def boom(*a, **k):
        raise AssertionError("the curve was evaluated")
    monkeypatch.setattr(frame_grabber.np, "floor", boom)
    assert np.array_equal(frame_grabber.levels_lut(16, 235, 1.0, 0, 1.0), M.linear_lut(16, 235))
    assert np.array_equal(frame_grabber.levels_lut(16, 235, gamma=1, brightness=0.0, contrast=1), M.linear_lut(16, 235))
    with pytest.raises(AssertionError):
        frame_grabber.levels_lut(16, 235, 1.0, 0, 1.5)


CURVES = [(2.2, 0, 1.0), (0.45, 0, 1.0), (1.0, 40, 1.0), (1.0, -40, 1.0), (1.0, 0, 1.5), (1.0, 0, 0.5), (1.0, 0, 0.0), (1.8, 12, 1.3),
          (0.6, -30, 2.5), (1.0, 255, 1.0), (1.0, -255, 1.0), (5.0, 0, 8.0)]


@pytest.mark.parametrize("gamma,brightness,contrast", CURVES)
def test_levels_lut_is_monotone_and_equals_the_model(gamma, brightness, contrast):
    import frame_grabber
    for black, white in ((0, 255), (16, 235), (64, 160), (0, 1), (254, 255), (100, 101)):
        lut = frame_grabber.levels_lut(black, white, gamma, brightness, contrast)
        assert lut.dtype == np.uint8 and np.array_equal(lut, M.levels_lut(black, white, gamma, brightness, contrast))
        assert (np.diff(lut.astype(int)) >= 0).all(), (black, white)
    # the curve alone: the ends of gamma are fixed, brightness shifts, contrast 0 is mid-grey
    if brightness == 0 and contrast == 1.0:
        c = M.curve(gamma, 0, 1.0)
        assert c[0] == 0 and c[255] == 255 and (c[128] > 128) == (gamma > 1)
    if contrast == 0.0:
        assert (M.curve(gamma, brightness, 0.0) == 128).all()


def test_levels_lut_refusals():
    import frame_grabber
    for bad in (dict(black=10, white=10), dict(black=11, white=10), dict(black=-1), dict(white=256), dict(gamma=0), dict(gamma=-1.0),
                dict(contrast=-0.1), dict(brightness=256), dict(gamma=float("nan")), dict(gamma=float("inf"))):
        with pytest.raises(ValueError):
            frame_grabber.levels_lut(**bad)
    for bad in (-1, 1025, 0.5):
        with pytest.raises(ValueError):
            frame_grabber.saturation_matrix(bad)
    for bad in (dict(saturation=4.5), dict(auto=(1,)), dict(auto=(0, 500001)), dict(per_channel=True), dict(auto_frames=2),
                dict(auto=True, black=5), dict(auto=True, auto_frames=0), dict(gamma=0)):
        with pytest.raises(ValueError):
            frame_grabber.Levels(**bad)
    assert frame_grabber.Levels(auto=True).auto == (5000, 5000) == native_ppm()


def native_ppm():
    import _iiv_native
    return _iiv_native.LEVELS_PPM


def test_saturation_matrix_for_every_s256():
    import frame_grabber
    greys = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    for s in range(1025):
        m = frame_grabber.saturation_matrix(s)
        assert m.dtype == np.int16 and m.shape == (3, 3) and np.array_equal(m, M.saturation_matrix(s))
        assert (m.astype(int).sum(axis=1) == 256).all(), s
        assert int(m.min()) >= -2048 and int(m.max()) <= 2047
        if s % 64 == 0 or s in (1, 255, 257, 1023):
            assert np.array_equal(M.apply(greys, M.IDENTITY_LUT, m), greys), s       # greys are fixed points
    assert np.array_equal(frame_grabber.saturation_matrix(256), M.IDENTITY_MATRIX)
    m0 = frame_grabber.saturation_matrix(0)
    assert (m0 == m0[0]).all() and m0[0].tolist() == [77, 150, 29]
    rgb = np.random.default_rng(1502).integers(0, 256, (500, 3)).astype(np.uint8)
    grey = M.apply(rgb, M.IDENTITY_LUT, m0)
    assert (grey[:, 0] == grey[:, 1]).all() and (grey[:, 1] == grey[:, 2]).all() and np.array_equal(grey[:, 0], M.luma(rgb))


# ---- the model's own properties ------------------------------------------------------------------------------------------------------

def test_model_identity_clamps_and_counts():
    x = LC.clip("noise", 260)
    assert np.array_equal(M.apply(x, M.IDENTITY_LUT, M.IDENTITY_MATRIX), x) and np.array_equal(LC.want_apply("noise", 260, "identity"), x)
    hi, lo = LC.want_apply("noise", 260, "max"), LC.want_apply("noise", 260, "min")
    total = x.astype(np.int64).sum(axis=-1, keepdims=True)
    assert np.array_equal(hi, np.broadcast_to(np.minimum((2047 * total + 128) >> 8, 255), x.shape)) and (hi == 255).mean() > 0.99
    assert (lo == 0).all() and ((-2048 * total + 128) >> 8).max() <= 0
    # 3 * 2047 * 255 and 3 * -2048 * 255 stay far inside int32
    assert 3 * 2048 * 255 + 128 < 2 ** 31
    for kind in LC.KINDS:
        h = LC.want_hist(kind, 260)
        assert h.shape == (LC.CLIPS, LC.FRAMES, 4, 256) and (h.astype(np.int64).sum(axis=-1) == 260).all()
    assert (LC.want_hist("flat", 1028).max(axis=-1) == 1028).all()                  # every lane on one bin
    assert ((LC.want_hist("two", 1028) > 0).sum(axis=-1) <= 2).all()
    e = LC.want_hist("extremes", 1028)
    assert e[0, 0, 3, 0] > 0 and e[0, 0, 3, 255] > 0 and e[0, 0, 3, 0] + e[0, 0, 3, 255] == 1028      # Y = 0 and Y = 255
    assert (e[:, :, :3, 1:255] == 0).all()
    assert M.luma(np.array([255, 255, 255])) == 255 and M.luma(np.array([0, 0, 0])) == 0
    # the random tables clamp on both sides and the near-identity ones on most bytes do not
    r = LC.want_apply("noise", 1028, "random")
    assert (r == 0).any() and (r == 255).any() and ((r > 0) & (r < 255)).any()
    s = LC.want_apply("noise", 1028, "small")
    assert ((s > 0) & (s < 255)).mean() > 0.7


def test_a_squeezed_ramp_comes_back(native):
    """a grey ramp squeezed into 64..160, through histogram model -> iiv_levels_auto -> levels_lut -> apply model: within one level
    of the ramp it came from"""
    import frame_grabber
    ramp = np.repeat((np.arange(53760) * 256 // 53760).astype(np.uint8)[:, None], 3, axis=1)
    squeezed = ((ramp.astype(np.int64) * (2 * 96) + 255) // 510 + 64).astype(np.uint8)
    assert squeezed.min() == 64 and squeezed.max() == 160
    hist = M.histogram(squeezed)
    assert np.array_equal(hist[3], hist[0])                                          # a grey's luma is the grey
    for ppm in ((0, 0), (5000, 5000)):
        black, white = native.levels_auto(hist[3], *ppm)
        assert (black, white) == M.auto(hist[3], *ppm)
        assert (black, white) == (64, 160)     # each end level holds half a level's share of 53760 pixels: 277, above k = 268
        back = M.apply(squeezed, frame_grabber.levels_lut(black, white))
        assert int(np.abs(back.astype(int) - ramp.astype(int)).max()) <= 1, ppm
        assert back.min() == 0 and back.max() == 255


# ---- the entry points' host side ----------------------------------------------------------------------------------------------------

def test_the_entry_points_are_declared_and_exported(native):
    for name, n_args in (("iiv_levels_histogram", 8), ("iiv_levels_auto", 5), ("iiv_levels_apply", 14)):
        assert name in native.SYMBOLS
        f = getattr(native.lib(), name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args
    assert native.lib().iiv_levels_apply.argtypes[2] is C.c_long and native.lib().iiv_levels_auto.argtypes[1] is C.c_uint32


def test_kernel_refusals_need_no_device(native):
    """every refusal of the header, with pointers that are never followed: the library decides before anything is launched"""
    L = native.lib()
    base = 1 << 20

    def hist(c=2, n=3, pixels=8, src=base, scs=96, sfs=24, out=base + 4096):
        return L.iiv_levels_histogram(c, n, pixels, C.c_void_p(src), scs, sfs, C.c_void_p(out), None)
    refused = [hist(c=-1), hist(n=-1), hist(pixels=0), hist(pixels=-4), hist(pixels=6), hist(pixels=9),
               hist(pixels=2 ** 31 + 4, sfs=3 * 2 ** 31 + 12, scs=9 * 2 ** 31 + 36),
               hist(src=base + 2), hist(out=base + 4097), hist(scs=98), hist(sfs=26), hist(sfs=20), hist(src=0), hist(out=0)]
    assert refused == [native.ERR_INVALID] * len(refused)
    assert b"iiv_levels_histogram" in L.iiv_last_error()
    assert hist(c=0) == 0 and hist(n=0) == 0 and hist(c=0, src=0, out=0) == 0

    def apply(c=2, n=3, pixels=8, src=base, scs=96, sfs=24, out=base + 4096, ocs=96, ofs=24, lut=base + 8192, ls=768, m=base + 16384,
              ms=20):
        return L.iiv_levels_apply(c, n, pixels, C.c_void_p(src), scs, sfs, C.c_void_p(out), ocs, ofs, C.c_void_p(lut), ls,
                                  C.c_void_p(m), ms, None)
    refused = [apply(c=-1), apply(n=-1), apply(pixels=0), apply(pixels=-4), apply(pixels=6), apply(pixels=9),
               apply(pixels=2 ** 40 + 4, sfs=3 * 2 ** 40 + 12, ofs=3 * 2 ** 40 + 12),
               apply(src=base + 2), apply(out=base + 4097), apply(lut=base + 8193), apply(m=base + 16386),
               apply(scs=98), apply(sfs=26), apply(ocs=94), apply(ofs=30), apply(ls=770), apply(ms=22),
               apply(sfs=20), apply(ofs=20), apply(ls=764), apply(ls=4), apply(ms=16), apply(ms=4),
               apply(src=0), apply(out=0), apply(lut=0), apply(m=0)]
    assert refused == [native.ERR_INVALID] * len(refused)
    assert b"iiv_levels_apply" in L.iiv_last_error()
    assert apply(c=0) == 0 and apply(n=0) == 0 and apply(c=0, src=0, out=0, lut=0, m=0) == 0
    assert apply(c=0, ls=0, ms=0) == 0 and apply(n=0, ls=772, ms=24) == 0


def test_levels_tables_checks_the_matrix_range(native):
    lut, m, ls, ms = native.levels_tables(M.IDENTITY_LUT, None, 3)
    assert lut.shape == (1, 3, 256) and (lut == M.IDENTITY_LUT).all() and (ls, ms) == (0, 0)
    assert m.dtype == np.int16 and m.shape == (1, 10) and m[0].tolist() == [256, 0, 0, 0, 256, 0, 0, 0, 256, 0]
    luts, ms_ = LC.tables("random")
    lut, m, ls, ms = native.levels_tables(luts, ms_, 3)
    assert (ls, ms) == (768, 20) and lut.shape == (3, 3, 256) and np.array_equal(m[:, :9].reshape(3, 3, 3), ms_) and (m[:, 9] == 0).all()
    for bad in (np.full((3, 3), 2048), np.full((3, 3), -2049), np.full((3, 3), 1.0), np.zeros((2, 3, 3), np.int64), np.zeros((3, 2), np.int64)):
        with pytest.raises(ValueError):
            native.levels_tables(M.IDENTITY_LUT, bad, 3)
    for bad in (np.zeros(255, np.uint8), np.zeros(256, np.int32), np.zeros((2, 3, 256), np.uint8)):
        with pytest.raises(ValueError):
            native.levels_tables(bad, None, 3)
