"""GPU: iiv_resize_frames_yuv420 (include/iivision.h f11; csrc/iiv_resize.hip) -- 4:2:0 planes into the device resize -- equals
resize_model.resize(yuv_model.to_rgb(...)) byte for byte: at the smallest shapes that take each path of the host code and the
kernels (two passes, one pass, none; the two-row and the one-row workgroup; the unfused paths), in every plane layout (I420,
NV12, NV21, padded rows at every offset mod 4, padded frames, planes cut out of a larger allocation), under the three preset
matrices and one at the argument bounds; then the refusals, the stream contract and the agreement with the RGB entry point."""
import ctypes as C

import numpy as np
import pytest

import resize_model
import yuv_model
from stream_probe import Probe

pytestmark = pytest.mark.gpu

# (h, w, H, W, frames)
SHAPES = [(7, 9, 5, 6, 3), (8, 33, 3, 7, 3),
          (9, 35, 4, 35, 3),            # vertical only: the unfused path
          (6, 10, 6, 4, 3),             # horizontal only
          (5, 5, 5, 5, 3),              # conversion only
          (1, 1, 1, 1, 3),
          (2, 4098, 2, 8, 1),           # w > 4096: one row per workgroup
          (48, 64, 192, 280, 3), (48, 64, 192, 560, 3),   # the real targets
          (202, 2, 4, 2, 3),            # h > 100 w
          (202, 2, 4, 3, 3)]            # h > 100 w and the width changes too: the vertical pass first, unfused
BOUNDS_MATRIX = (255, 1023, -1023, 1023, -1023, 1023)
_cache = {}


def _planes(h, w, n, extremes=False):
    key = ("planes", h, w, n, extremes)
    if key not in _cache:
        y, u, v = yuv_model.random_planes(n, h, w, seed=1000 * h + w)
        if extremes:
            y, u, v = ((p >> 7) * np.uint8(255) for p in (y, u, v))   # planes holding 0 and 255
        _cache[key] = tuple(np.ascontiguousarray(p) for p in (y, u, v))
        for p in _cache[key]:
            p.setflags(write=False)
    return _cache[key]


def _expected(h, w, H, W, n, matrix="bt601", extremes=False):
    key = ("exp", h, w, H, W, n, matrix, extremes)
    if key not in _cache:
        _cache[key] = resize_model.resize(yuv_model.to_rgb(*_planes(h, w, n, extremes), matrix), (H, W))
        _cache[key].setflags(write=False)
    return _cache[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("h,w,H,W,n", SHAPES)
def test_device_equals_model(native, h, w, H, W, n):
    y, u, v = _planes(h, w, n)
    got = native.resize_frames_yuv420(_dev(y), _dev(u), _dev(v), (H, W))
    assert tuple(got.shape) == (n, H, W, 3)
    assert np.array_equal(_np(got), _expected(h, w, H, W, n))


def _filled(shape, fill):
    import torch
    return torch.full(shape, fill, dtype=torch.uint8, device="cuda")


def _layout(name, y, u, v, fill=0xFF):
    """the planes on the device as views in layout `name`; everything around them holds `fill`"""
    import torch
    n, h, w = y.shape
    _, ch, cw = u.shape
    if name == "i420":
        return _dev(y), _dev(u), _dev(v)
    if name in ("nv12", "nv21"):
        uv = _dev(np.stack([u, v] if name == "nv12" else [v, u], axis=-1))
        return (_dev(y), uv[..., 0], uv[..., 1]) if name == "nv12" else (_dev(y), uv[..., 1], uv[..., 0])
    if name == "rows":       # row strides = 1 mod 4: consecutive rows start at every byte offset mod 4
        ys, cs = w + (1 - w) % 4 + 4, cw + (1 - cw) % 4
        assert ys % 4 == 1 and cs % 4 == 1
        by, bu, bv = _filled((n, h, ys), fill), _filled((n, ch, cs), fill), _filled((n, ch, cs), fill)
        vy, vu, vv = by[:, :, :w], bu[:, :, :cw], bv[:, :, :cw]
    elif name == "nv12_rows":   # the same for the interleaved plane: a row stride of 2 cw + 1, 2 cw + 3 ... = 1 mod 4 bytes
        ys, cs = w + (1 - w) % 4, 2 * cw + (1 - 2 * cw) % 4
        by, buv = _filled((n, h, ys), fill), _filled((n, ch, cs), fill)
        vy = by[:, :, :w]
        vu = torch.as_strided(buv, (n, ch, cw), (ch * cs, cs, 2))
        vv = torch.as_strided(buv, (n, ch, cw), (ch * cs, cs, 2), storage_offset=1)
    elif name == "frames":   # a padded frame stride
        by, bu, bv = _filled((n, h + 3, w), fill), _filled((n, ch + 1, cw), fill), _filled((n, ch + 1, cw), fill)
        vy, vu, vv = by[:, :h], bu[:, :ch], bv[:, :ch]
    elif name == "cut":      # planes cut out of a larger allocation, odd offsets on every side
        by, bu, bv = _filled((n + 2, h + 2, w + 5), fill), _filled((n + 2, ch + 2, cw + 5), fill), _filled((n + 2, ch + 2, cw + 5), fill)
        vy, vu, vv = by[1:1 + n, 1:1 + h, 3:3 + w], bu[1:1 + n, 1:1 + ch, 1:1 + cw], bv[1:1 + n, 1:1 + ch, 2:2 + cw]
    elif name == "nv12_cut":
        by, buv = _filled((n + 2, h + 2, w + 5), fill), _filled((n + 2, ch + 2, cw + 3, 2), fill)
        vy = by[1:1 + n, 1:1 + h, 3:3 + w]
        vu, vv = buv[1:1 + n, 1:1 + ch, 1:1 + cw, 0], buv[1:1 + n, 1:1 + ch, 1:1 + cw, 1]
    else:
        raise KeyError(name)
    vy.copy_(_dev(y))
    vu.copy_(_dev(u))
    vv.copy_(_dev(v))
    return vy, vu, vv


LAYOUTS = ["i420", "nv12", "nv21", "rows", "nv12_rows", "frames", "cut", "nv12_cut"]


# fused two passes, unfused, fused one pass, unfused with the vertical pass first
@pytest.mark.parametrize("h,w,H,W", [(7, 9, 5, 6), (9, 35, 4, 35), (8, 33, 8, 7), (202, 2, 4, 3)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts(native, layout, h, w, H, W):
    y, u, v = _planes(h, w, 3)
    exp = _expected(h, w, H, W, 3)
    for fill in (0xFF, 0x00):    # nothing outside the planes influences the result
        got = native.resize_frames_yuv420(*_layout(layout, y, u, v, fill), (H, W))
        assert np.array_equal(_np(got), exp), (layout, fill)


@pytest.mark.parametrize("matrix", ["bt601", "bt709", "jpeg", (16, 298, 409, -100, -208, 516)])
def test_preset_matrices(native, matrix):
    y, u, v = _planes(7, 9, 3)
    got = native.resize_frames_yuv420(_dev(y), _dev(u), _dev(v), (5, 6), matrix=matrix)
    assert np.array_equal(_np(got), _expected(7, 9, 5, 6, 3, matrix))


@pytest.mark.parametrize("h,w,H,W", [(7, 9, 5, 6), (5, 5, 5, 5)])
def test_matrix_at_the_bounds(native, h, w, H, W):
    y, u, v = _planes(h, w, 3, extremes=True)
    assert set(np.unique(y)) <= {0, 255}
    got = native.resize_frames_yuv420(_dev(y), _dev(u), _dev(v), (H, W), matrix=BOUNDS_MATRIX)
    assert np.array_equal(_np(got), _expected(h, w, H, W, 3, BOUNDS_MATRIX, extremes=True))


def _raw(native, n, h, w, H, W, ps=1, matrix=yuv_model.MATRICES["bt601"]):
    """one call of the C ABI on buffers large enough for any of the shapes below -> (return code, the output)"""
    import torch
    y, u, v = (_filled((4096,), 7) for _ in range(3))
    dst = _filled((n * H * W * 3 + 16,), 0xA5)
    m = np.asarray(matrix, np.int32)
    cw, ch = max((w + 1) // 2, 1), (h + 1) // 2
    rc = native.lib().iiv_resize_frames_yuv420(n, h, w, native.dptr(y), h * w, w, native.dptr(u), native.dptr(v), ch * cw * ps, cw * ps,
                                               ps, m.ctypes.data_as(C.c_void_p), H, W, native.dptr(dst), native.stream_ptr())
    torch.cuda.synchronize()
    return rc, _np(dst)


def test_refusals_launch_nothing(native):
    rc, dst = _raw(native, 2, 6, 8, 3, 4)
    assert rc == native.OK and not (dst[:2 * 3 * 4 * 3] == 0xA5).all() and (dst[2 * 3 * 4 * 3:] == 0xA5).all()
    for kw in (dict(ps=3), dict(ps=0), dict(matrix=(16, 1024, 409, -100, -208, 516)), dict(matrix=(16, 298, 409, -100, -1024, 516)),
               dict(matrix=(256, 298, 409, -100, -208, 516)), dict(matrix=(-1, 298, 409, -100, -208, 516))):
        rc, dst = _raw(native, 2, 6, 8, 3, 4, **kw)
        assert rc == native.ERR_INVALID and (dst == 0xA5).all(), kw
        assert b"iiv_resize_frames_yuv420" in native.lib().iiv_last_error()
    for (h, w, H, W) in ((6, 0, 3, 4), (0, 8, 3, 4), (6, 8, 1025, 4), (6, 8, 3, 1025), (6, 8, 0, 4)):
        rc, dst = _raw(native, 2, h, w, H, W)
        assert rc == native.ERR_INVALID and (dst == 0xA5).all(), (h, w, H, W)
    # overlapping rows, a NULL plane, a NULL matrix
    import torch
    y, out = _filled((4096,), 7), _filled((2 * 3 * 4 * 3,), 0xA5)
    m = np.asarray(yuv_model.MATRICES["bt601"], np.int32).ctypes.data_as(C.c_void_p)
    L, p, st = native.lib(), native.dptr(y), native.stream_ptr()
    assert L.iiv_resize_frames_yuv420(2, 6, 8, p, 48, 7, p, p, 12, 4, 1, m, 3, 4, native.dptr(out), st) == native.ERR_INVALID
    assert L.iiv_resize_frames_yuv420(2, 6, 8, p, 48, 8, p, p, 12, 3, 1, m, 3, 4, native.dptr(out), st) == native.ERR_INVALID
    assert L.iiv_resize_frames_yuv420(2, 6, 8, p, 48, 8, p, p, 11, 4, 1, m, 3, 4, native.dptr(out), st) == native.ERR_INVALID
    assert L.iiv_resize_frames_yuv420(2, 6, 8, p, 48, 8, p, p, 24, 8, 2, m, 3, 4, native.dptr(out), st) == native.OK
    assert L.iiv_resize_frames_yuv420(2, 6, 8, p, 48, 8, p, p, 24, 6, 2, m, 3, 4, native.dptr(out), st) == native.ERR_INVALID
    assert L.iiv_resize_frames_yuv420(2, 6, 8, p, 48, 8, None, p, 12, 4, 1, m, 3, 4, native.dptr(out), st) == native.ERR_INVALID
    assert L.iiv_resize_frames_yuv420(2, 6, 8, p, 48, 8, p, p, 12, 4, 1, None, 3, 4, native.dptr(out), st) == native.ERR_INVALID
    assert L.iiv_resize_frames_yuv420(0, 6, 8, None, 0, 0, None, None, 0, 0, 1, m, 3, 4, None, st) == native.OK      # no frame: nothing to do
    torch.cuda.synchronize()


def test_python_checks_shapes_and_strides(native):
    y, u, v = (_dev(p) for p in _planes(7, 9, 3))
    with pytest.raises(ValueError, match=r"\(3, 4, 5\)"):       # the expected chroma shape is named
        native.resize_frames_yuv420(y, u[:, :, :4], v[:, :, :4], (5, 6))
    with pytest.raises(ValueError, match=r"\(3, 4, 5\)"):
        native.resize_frames_yuv420(y, u, v[:, :3], (5, 6))
    with pytest.raises(ValueError):
        native.resize_frames_yuv420(y.cpu(), u, v, (5, 6))
    with pytest.raises(ValueError):
        native.resize_frames_yuv420(y, u, _dev(np.stack([_planes(7, 9, 3)[2]] * 2, -1))[..., 0], (5, 6))   # u planar, v interleaved
    with pytest.raises(ValueError):
        native.resize_frames_yuv420(y, u, v, (5, 6), matrix="bt2020")
    with pytest.raises(native.IIVError):
        native.resize_frames_yuv420(y, u, v, (5, 6), matrix=(16, 1024, 0, 0, 0, 0))


def test_side_stream_under_the_probe(native):
    """The call on a busy non-blocking side stream, the host matrix overwritten right after it returns (tests/stream_probe.py)."""
    L = native.lib()
    h, w, H, W, n = 48, 64, 192, 280, 3
    ry, ru, rv = _planes(h, w, n)
    p = Probe()
    y, u, v = p.input(ry, np.roll(ry, 1, axis=0)), p.input(ru, np.roll(ru, 1, axis=0)), p.input(rv, np.roll(rv, 1, axis=0))
    dst = p.output((n, H, W, 3))
    m = p.host(np.asarray(yuv_model.MATRICES["bt601"], np.int32), np.asarray(yuv_model.MATRICES["jpeg"], np.int32))
    ch, cw = (h + 1) // 2, (w + 1) // 2

    def call(st):
        native.check(L.iiv_resize_frames_yuv420(n, h, w, native.dptr(y), h * w, w, native.dptr(u), native.dptr(v), ch * cw, cw, 1,
                                                m.ctypes.data_as(C.c_void_p), H, W, native.dptr(dst), st))
    call(native.stream_ptr())                     # the first use of a size pair uploads its tables
    p.run(call)
    assert np.array_equal(_np(dst), _expected(h, w, H, W, n))


def test_a_seen_size_pair_does_not_wait_for_the_stream(native):
    import torch
    h, w, H, W, n = 48, 64, 192, 280, 3
    y, u, v = (_dev(p) for p in _planes(h, w, n))
    exp = _expected(h, w, H, W, n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out1 = native.resize_frames_yuv420(y, u, v, (H, W))      # (may be the first use of 64 -> 280 / 48 -> 192: uploads)
    side.synchronize()
    assert np.array_equal(_np(out1), exp)
    out2 = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(200_000_000)                  # keeps the side stream busy for tens of milliseconds
        native.resize_frames_yuv420(y, u, v, (H, W), out=out2)
        busy = not side.query()                         # the call returned while the stream was still sleeping
    assert busy, "a second call with the same size pair synchronised the host"
    side.synchronize()
    assert np.array_equal(_np(out2), exp)


def test_agrees_with_the_rgb_entry_point(native):
    h, w, H, W, n = 48, 64, 192, 280, 3
    y, u, v = _planes(h, w, n)
    rgb = _dev(yuv_model.to_rgb(y, u, v, "bt601"))
    got = native.resize_frames_yuv420(_dev(y), _dev(u), _dev(v), (H, W))
    assert np.array_equal(_np(got), _np(native.resize_frames(rgb, (H, W))))


def test_frame_grabber_takes_the_triple(native):
    import frame_grabber
    import palette
    import video_mode
    h, w, n = 48, 64, 3
    y, u, v = (p.copy() for p in _planes(h, w, n))
    nv12 = np.stack([u, v], axis=-1)
    for vm, pal, size in ((video_mode.VideoMode.DHGR, palette.Palette.NTSC, (192, 280)), (video_mode.VideoMode.DHGR, palette.Palette.MONO, (192, 560)),
                          (video_mode.VideoMode.HGR, palette.Palette.MONO, (192, 280))):
        exp_rgb = np.array(_expected(h, w, size[0], size[1], n))   # (a writable copy: the grabber uploads it as it is)
        for planes in ((y, u, v), (y, nv12[..., 0], nv12[..., 1])):
            got = frame_grabber.ArrayFrameGrabber(planes, vm, pal, resize=True, yuv_matrix="bt601", batch=2)
            assert np.array_equal(_np(got.ingest_frames()), exp_rgb)
            exp = frame_grabber.ArrayFrameGrabber(exp_rgb, vm, pal)
            for (m1, a1), (m2, a2) in zip(got.frames(), exp.frames()):     # batched: frames 0-1, then 2
                assert np.array_equal(m1.page_offset, m2.page_offset)
                assert (a1 is None and a2 is None) or np.array_equal(a1.page_offset, a2.page_offset)
    with pytest.raises(ValueError):
        frame_grabber.ArrayFrameGrabber((y, u, v), video_mode.VideoMode.DHGR)                    # a triple needs resize=True
    with pytest.raises(ValueError):
        frame_grabber.ArrayFrameGrabber((y, u[:, :, :-1], v), video_mode.VideoMode.DHGR, resize=True)
