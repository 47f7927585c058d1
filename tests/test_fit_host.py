"""CPU: f12 without a device -- the tests' model of the boxed resize (tests/fit_model.py) against the installed Pillow and against
Pillow's recorded output (tests/golden/g12_fit.npz), iiv_resize_coeffs_box against the model's tables entry for entry,
frame_grabber.fit_geometry's pinned values and invariants, and the argument errors of the Python wrappers."""
import zlib

import numpy as np
import pytest

import fit_cases as FC
import fit_model as FM
import resize_model


def _f32(box):
    return tuple(float(np.float32(v)) for v in box)


@pytest.mark.parametrize("name", FC.GOLDEN)
def test_model_is_the_recorded_pillow(golden, name):
    _, h, w, box, size, rect = FC.case(name)
    g = golden.g12_fit
    src = FC.source(name)
    assert zlib.crc32(src.tobytes()) == int(g["crc_" + name]), "the seeded source is not the frame the golden was recorded from"
    assert tuple(g["fill"]) == FC.FILL
    assert np.array_equal(FM.fit(src, box, size, rect, FC.FILL), g["dst_" + name])


def test_golden_holds_every_listed_case(golden):
    assert list(golden.g12_fit["names"]) == FC.GOLDEN and set(FC.GOLDEN) <= set(FC.NAMES)


def test_model_is_the_installed_pillow():
    """seeded random cases: fractional boxes, integer boxes, boxes spanning an axis, tall thin sources on both sides of the
    pass-order rule -- and every fit_cases case"""
    pytest.importorskip("PIL")
    rng = np.random.RandomState(12)
    n = 0
    for i in range(150):
        if i % 10 == 0:
            w = int(rng.randint(1, 4))
            h = 100 * w + int(rng.randint(-3, 4))   # h > 100 w decides the order
        else:
            h, w = (int(v) for v in rng.randint(1, 90, 2))
        size = tuple(int(v) for v in rng.randint(1, 48, 2))
        box, rect = FC.random_geometry(rng, h, w, *size)
        a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        assert np.array_equal(FM.fit(a, box, size, rect, FC.FILL), FM.pillow_fit(a, box, size, rect, FC.FILL)), (h, w, box, size, rect)
        n += 1
    for name in FC.NAMES:
        _, h, w, box, size, rect = FC.case(name)
        assert np.array_equal(FM.fit(FC.source(name), box, size, rect, FC.FILL),
                              FM.pillow_fit(FC.source(name), _f32(box), size, rect, FC.FILL)), name
    assert n == 150


def test_whole_box_is_the_plain_model():
    for h, w, H, W in [(37, 53, 24, 40), (301, 2, 24, 5), (24, 40, 24, 40), (5, 7, 3, 2)]:
        a = np.random.RandomState(h).randint(0, 256, (h, w, 3)).astype(np.uint8)
        assert np.array_equal(FM.resize_box(a, (0, 0, w, h), (H, W)), resize_model.resize(a, (H, W)))
        assert all(np.array_equal(p, q) for p, q in zip(FM.coeffs_box(h, 0, h, H)[1:], resize_model.coeffs(h, H)[1:]))


# (in_size, in0, in1, out_size): 0.1 + 52.6 etc. are no float32 values, and the third's float32 extent differs from its float64 one
COEFF_CASES = [(53, 0.1, 52.7, 37), (37, 0.3, 36.9, 22), (1080, 13.3, 1071.9, 192), (1920, 240, 1680, 280), (854, 107, 747, 280),
               (53, 20.25, 20.75, 5), (53, 10, 30, 20), (8192, 0.7, 8191.2, 1024), (11, 3, 8, 10), (2, 0.5, 2, 9), (480, 0, 480, 192)]


def test_a_float32_extent_differs_from_the_float64_one():
    """the case list holds a box whose extent, subtracted in float32 as Pillow does, is not the float64 difference of its
    float32 ends -- and whose table changes with it"""
    differing = 0
    for in_size, in0, in1, out in COEFF_CASES:
        a, b = np.float32(in0), np.float32(in1)
        if float(b - a) != float(b) - float(a):
            differing += 1
    assert differing >= 1


@pytest.mark.parametrize("in_size,in0,in1,out", COEFF_CASES)
def test_library_coefficients_are_the_models(native, in_size, in0, in1, out):
    """iiv_resize_coeffs_box (host only) against the model, entry for entry"""
    ksize, bounds, k = FM.coeffs_box(in_size, in0, in1, out)
    got_bounds, got_k = native.resize_coeffs_box(in_size, in0, in1, out)
    assert got_k.shape == (out, ksize)
    assert np.array_equal(got_bounds, bounds) and np.array_equal(got_k, k)


def test_library_coefficients_of_the_whole_axis_are_the_plain_ones(native):
    for in_size, out in [(1080, 192), (53, 280), (7, 7), (8192, 1)]:
        for p, q in zip(native.resize_coeffs_box(in_size, 0, in_size, out), native.resize_coeffs(in_size, out)):
            assert np.array_equal(p, q)


def test_library_refuses_a_bad_axis_box(native):
    for in0, in1 in [(-0.5, 10), (5, 5), (6, 5), (0, 53.5), (float("nan"), 10)]:
        with pytest.raises(native.IIVError) as e:
            native.resize_coeffs_box(53, in0, in1, 20)
        assert e.value.code == native.ERR_INVALID and "iiv_resize_coeffs_box" in str(e.value)


# ---- fit_geometry ----------------------------------------------------------------------------------------------------------

def test_pinned_geometry():
    from frame_grabber import fit_geometry
    whole = lambda h, w, W=280: ((0.0, 0.0, float(w), float(h)), (0, 0, W, 192))
    assert fit_geometry(1080, 1920, 192, 280, "letterbox") == (whole(1080, 1920)[0], (0, 24, 280, 144))
    assert fit_geometry(1080, 1920, 192, 280, "crop") == ((240.0, 0.0, 1680.0, 1080.0), (0, 0, 280, 192))
    assert fit_geometry(480, 854, 192, 280, "letterbox")[1][3] == 144
    assert fit_geometry(480, 854, 192, 280, "crop")[0] == (107.0, 0.0, 747.0, 480.0)
    assert fit_geometry(480, 720, 192, 280, "letterbox", sar=(32, 27))[1][3] == 144
    for fit in ("stretch", "letterbox", "crop"):
        assert fit_geometry(480, 720, 192, 280, fit, sar=(8, 9)) == whole(480, 720)
        assert fit_geometry(480, 640, 192, 280, fit) == whole(480, 640)
        assert fit_geometry(480, 640, 192, 560, fit) == whole(480, 640, 560)
    # the 560-dot mono screen shows the same picture: the same rows, twice the columns
    assert fit_geometry(1080, 1920, 192, 560, "letterbox")[1] == (0, 24, 560, 144)
    # a portrait source, display aspect 9:16 = 27/64 of 4:3: 280 * 27 / 64 = 118.1 columns -> 118 (even), 81 on either side;
    # the crop keeps 1920 * 27 / 64 = 810 of its rows
    assert fit_geometry(1920, 1080, 192, 280, "letterbox")[1] == (81, 0, 118, 192)
    assert fit_geometry(1920, 1080, 192, 280, "crop")[0] == (0.0, 555.0, 1080.0, 1365.0)


def test_geometry_invariants_over_a_seeded_sweep():
    from frame_grabber import fit_geometry
    import random
    r = random.Random(12)
    for _ in range(2000):
        h, w, H, W = r.randint(1, 4000), r.randint(1, 4000), r.randint(1, 300), r.randint(1, 600)
        sar = (r.randint(1, 40), r.randint(1, 40))
        assert fit_geometry(h, w, H, W, "stretch", sar) == ((0.0, 0.0, float(w), float(h)), (0, 0, W, H))
        for fit in ("letterbox", "crop"):
            box, rect = fit_geometry(h, w, H, W, fit, sar)
            assert (box, rect) == FM.fit_geometry(h, w, H, W, fit, sar)
            x0, y0, x1, y1 = box
            assert all(float(np.float32(v)) == v for v in box)
            assert 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h
            rx, ry, rw, rh = rect
            assert rx >= 0 and ry >= 0 and rw >= 1 and rh >= 1 and rx + rw <= W and ry + rh <= H
            if fit == "letterbox":
                assert box == (0.0, 0.0, float(w), float(h)) and (rw == W or rh == H)
                assert rw == W or rw % 2 == 0 or W == 1
                assert abs((W - rw) - 2 * rx) <= 1 and abs((H - rh) - 2 * ry) <= 1   # centred
            else:
                assert rect == (0, 0, W, H) and (x1 - x0 == w or y1 - y0 == h)
                assert abs((x0 + x1) - w) < 1e-3 * w + 1e-3 and abs((y0 + y1) - h) < 1e-3 * h + 1e-3


def test_geometry_refuses_bad_arguments():
    from frame_grabber import fit_geometry
    for args in [(480, 640, 192, 280, "pad"), (0, 640, 192, 280, "crop"), (480, 640, 192, 280, "crop", (0, 1)),
                 (480, 640, 192, 280, "crop", (1, -1))]:
        with pytest.raises(ValueError):
            fit_geometry(*args)


# ---- the wrappers' argument errors --------------------------------------------------------------------------------------------

def test_fit_args(native):
    assert native.fit_args(37, 53, 24, 40) is None
    box, rect, fill = native.fit_args(37, 53, 24, 40, fill=(1, 2, 3))
    assert box.dtype == np.float32 and tuple(box) == (0, 0, 53, 37) and rect.dtype == np.int32 and tuple(rect) == (0, 0, 40, 24)
    assert fill == 1 | 2 << 8 | 3 << 16
    box, rect, fill = native.fit_args(37, 53, 24, 40, box=(0.1, 2, 50, 30.5), rect=(1, 2, 3, 4))
    assert tuple(box) == tuple(np.array((0.1, 2, 50, 30.5), np.float32)) and tuple(rect) == (1, 2, 3, 4) and fill == 0
    bad = [dict(box=(0, 0, 53)), dict(box="whole"), dict(box=(-1, 0, 53, 37)), dict(box=(0, 0, 53.5, 37)), dict(box=(5, 0, 5, 37)),
           dict(box=(0, 9, 53, 8)), dict(box=(0, 0, 53, 37.01)), dict(box=(0, 0, float("nan"), 37)),
           dict(rect=(0, 0, 40)), dict(rect=(0, 0, 41, 24)), dict(rect=(-1, 0, 4, 4)), dict(rect=(0, 0, 0, 4)), dict(rect=(38, 0, 3, 4)),
           dict(rect=(0, 21, 3, 4)), dict(rect=(0.5, 0, 3, 4)),
           dict(fill=(1, 2)), dict(fill=(1, 2, 256)), dict(fill=(-1, 2, 3)), dict(fill=7), dict(fill=(1.5, 2, 3))]
    for kw in bad:
        with pytest.raises(ValueError):
            native.fit_args(37, 53, 24, 40, **kw)


def test_frame_grabber_refuses_bad_fit_arguments():
    import frame_grabber as FG
    from video_mode import VideoMode
    frames = np.zeros((1, 54, 128, 3), np.uint8)
    with pytest.raises(ValueError, match="fit must be one of"):
        FG.ArrayFrameGrabber(frames, VideoMode.DHGR, resize=True, fit="pad")
    with pytest.raises(ValueError, match="resize=True"):
        FG.ArrayFrameGrabber(np.zeros((1, 192, 280, 3), np.uint8), VideoMode.DHGR, fit="crop")
    with pytest.raises(ValueError, match="fill"):
        FG.ArrayFrameGrabber(frames, VideoMode.DHGR, resize=True, fit="letterbox", fill=(0, 0, 300))
    with pytest.raises(ValueError, match="sar"):
        FG.ArrayFrameGrabber(frames, VideoMode.DHGR, resize=True, fit="letterbox", sar=(0, 1))
    g = FG.ArrayFrameGrabber(frames, VideoMode.DHGR, resize=True)
    assert g.fit == "stretch" and g._fit == {}
