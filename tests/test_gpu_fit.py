"""GPU: f12, the boxed resize into a rectangle of the destination (iiv_resize_frames_fit / iiv_resize_frames_yuv420_fit,
csrc/iiv_resize.hip), byte for byte against the tests' model (tests/fit_model.py) and against Pillow's own recorded output
(tests/golden/g12_fit.npz) on uint8 noise.  Every call writes into a destination that is prefilled with a sentinel and sits
between guard bytes at a varying alignment; the fill colour has three different bytes.  The geometries are fit_cases.CASES:
the smallest shapes at which a column window, a row window, an odd chroma offset, a rectangle's byte alignment, the pass order
or the unfused 4:2:0 path can go wrong.  Nothing here is ever out of range: the guards are compared, never crossed."""
import functools

import numpy as np
import pytest

import fit_cases as FC
import fit_model as FM
import resize_model
import yuv_model
from device_guards import guarded, guards_kept, ok
from stream_probe import Probe
from test_gpu_resize_batches import CHUNK_MID_BYTES, MAX_LAUNCH_ITEMS, P, _check_periodic

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 0x3C
LAYOUTS = ("i420", "nv12")


def _dst(n, size, lead):
    """a guarded, sentinel-prefilled destination of n frames -> (buffer, view, lead)"""
    nbytes = n * size[0] * size[1] * 3
    buf, view = guarded(nbytes, lead, 67, GUARD)
    view.fill_(SENTINEL)
    return buf, view


def _result(buf, view, lead, n, size):
    import torch
    torch.cuda.synchronize()
    assert guards_kept(buf, lead, view.numel(), GUARD), "bytes outside the destination were written"
    return view.cpu().numpy().reshape(n, size[0], size[1], 3)


def fit_rgb(native, src, box, size, rect, fill=FC.FILL, lead=16):
    """native.resize_frames(box=, rect=, fill=) of numpy (n, h, w, 3) into a guarded destination -> numpy (n, H, W, 3)"""
    import torch
    buf, view = _dst(len(src), size, lead)
    native.resize_frames(torch.from_numpy(np.ascontiguousarray(src)).cuda(), size, out=view, box=box, rect=rect, fill=fill)
    return _result(buf, view, lead, len(src), size)


def _device_planes(y, u, v, layout):
    import torch
    d_y = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    if layout == "nv12":
        uv = torch.from_numpy(np.ascontiguousarray(np.stack([u, v], -1))).cuda()
        return d_y, uv[..., 0], uv[..., 1]
    return d_y, torch.from_numpy(np.ascontiguousarray(u)).cuda(), torch.from_numpy(np.ascontiguousarray(v)).cuda()


def fit_yuv(native, planes, layout, box, size, rect, fill=FC.FILL, lead=16):
    buf, view = _dst(len(planes[0]), size, lead)
    native.resize_frames_yuv420(*_device_planes(*planes, layout), size=size, out=view, box=box, rect=rect, fill=fill)
    return _result(buf, view, lead, len(planes[0]), size)


@functools.lru_cache(maxsize=None)
def expected_rgb(name):
    _, h, w, box, size, rect = FC.case(name)
    return FM.fit(FC.source(name)[None], box, size, rect, FC.FILL)


@functools.lru_cache(maxsize=None)
def planes_of(name):
    _, h, w = FC.case(name)[:3]
    return yuv_model.random_planes(1, h, w, 2000 + FC.NAMES.index(name))


@functools.lru_cache(maxsize=None)
def expected_yuv(name):
    _, h, w, box, size, rect = FC.case(name)
    return FM.fit(yuv_model.to_rgb(*planes_of(name)), box, size, rect, FC.FILL)


def _same(got, exp):
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, "%d bytes differ from the model, the first at (frame, y, x, channel) %s: %d for %d" % (
        len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


@pytest.mark.parametrize("name", FC.NAMES)
def test_rgb_case(native, name):
    _, h, w, box, size, rect = FC.case(name)
    _same(fit_rgb(native, FC.source(name)[None], box, size, rect, lead=16 + FC.NAMES.index(name) % 4), expected_rgb(name))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", FC.NAMES)
def test_yuv_case(native, name, layout):
    """the box counts in the frame the planes define: chroma at absolute (y >> 1, x >> 1), odd offsets and odd sizes included"""
    _, h, w, box, size, rect = FC.case(name)
    _same(fit_yuv(native, planes_of(name), layout, box, size, rect, lead=16 + FC.NAMES.index(name) % 4), expected_yuv(name))


@pytest.mark.parametrize("name", FC.GOLDEN)
def test_rgb_case_is_pillows_own(native, golden, name):
    """the device against what Pillow itself made of the case (recorded: no Pillow is needed here)"""
    _, h, w, box, size, rect = FC.case(name)
    g = golden.g12_fit
    assert tuple(g["geo_" + name]) == tuple(float(v) for v in tuple(box) + tuple(size) + tuple(rect))
    _same(fit_rgb(native, FC.source(name)[None], box, size, rect)[0], g["dst_" + name])


def test_staged_windows_cover_every_alignment(native):
    """what the column cases are there for: the first staged column of the cols* cases falls in each residue of (3 cmin) mod 4,
    the rectangles' rx and rw in each residue too, and the wide case stages more than 4096 columns (one row a workgroup)"""
    rxs, rws = set(), set()
    for size in ("13x11", "37x53"):
        cmins = set()
        for k in range(4):
            _, h, w, box, _, rect = FC.case("cols%s_%d" % (size, k))
            bounds, _ = native.resize_coeffs_box(w, box[0], box[2], rect[2])
            cmins.add(3 * int(bounds[:, 0].min()) % 4)
            rxs.add(3 * rect[0] % 4)
            rws.add(3 * rect[2] % 4)
        assert cmins == {0, 1, 2, 3}
    assert rxs == rws == {0, 1, 2, 3}
    _, h, w, box, _, rect = FC.case("wide")
    bounds, _ = native.resize_coeffs_box(w, box[0], box[2], rect[2])
    assert int((bounds[:, 0] + bounds[:, 1]).max()) - int(bounds[:, 0].min()) > 4096
    assert resize_model.vertical_first(*FC.case("tall")[1:3])


def test_batch_with_frame_strides(native):
    """n = 3 frames cut out of a larger tensor: frame and row strides that are not the packed ones, a first byte that is not
    4-byte aligned; and padded planes for the 4:2:0 entry point"""
    import torch
    rng = np.random.RandomState(77)
    big = rng.randint(0, 256, (3, 50, 70, 3)).astype(np.uint8)
    box, size, rect = (5.25, 3.5, 50.75, 33.0), (24, 40), (3, 2, 31, 19)
    d_big = torch.from_numpy(big).cuda()
    view = d_big[:, 7:44, 9:62]
    assert view.stride(0) != 37 * 53 * 3 and view.stride(1) != 53 * 3 and view.storage_offset() % 4 != 0
    buf, out = _dst(3, size, 17)
    native.resize_frames(view, size, out=out, box=box, rect=rect, fill=FC.FILL)
    _same(_result(buf, out, 17, 3, size), FM.fit(big[:, 7:44, 9:62], box, size, rect, FC.FILL))
    y, u, v = yuv_model.random_planes(3, 37, 53, 78)
    py, pu, pv = (torch.full((3, p.shape[1] + 3, p.shape[2] + 5), 0xC7, dtype=torch.uint8, device="cuda") for p in (y, u, v))
    for pad, p in ((py, y), (pu, u), (pv, v)):
        pad[:, :p.shape[1], :p.shape[2]] = torch.from_numpy(p).cuda()
    buf, out = _dst(3, size, 18)
    native.resize_frames_yuv420(py[:, :37, :53], pu[:, :19, :27], pv[:, :19, :27], size=size, out=out, box=box, rect=rect, fill=FC.FILL)
    _same(_result(buf, out, 18, 3, size), FM.fit(yuv_model.to_rgb(y, u, v), box, size, rect, FC.FILL))


def test_past_the_first_scratch_chunk(native):
    """three tall narrow frames, horizontal pass first (8192 <= 100 * 82): the staged intermediate is all 8192 rows of 3000 bytes,
    24 MB a frame, so each frame is a chunk of its own and the second and third go through the loop's later trips"""
    h, w, size, rect = 8192, 82, (8, 1024), (11, 1, 1000, 6)
    box = (1.5, 96.0, 80.25, 8096.0)
    bounds, _ = native.resize_coeffs_box(h, box[1], box[3], rect[3])
    rows = int((bounds[:, 0] + bounds[:, 1]).max()) - int(bounds[:, 0].min())
    assert not resize_model.vertical_first(h, w) and 2 * rows * 3000 > CHUNK_MID_BYTES
    src = np.random.RandomState(79).randint(0, 256, (3, h, w, 3)).astype(np.uint8)
    _same(fit_rgb(native, src, box, size, rect), FM.fit(src, box, size, rect, FC.FILL))


def test_past_the_first_launch_piece(native):
    """as test_gpu_resize_batches.test_grid_limit: the vertical pass of a 1024-row rectangle is 1024 workgroups of 256 a
    frame, so 20000 frames do not fit one launch; frame i is base[i % 7]"""
    import torch
    n, h, w, size, rect, box = 20000, 1, 2, (1024, 2), (1, 0, 1, 1024), (0.25, 0.0, 1.75, 1.0)
    assert n * 1024 * 256 > MAX_LAUNCH_ITEMS
    base = np.random.RandomState(80).randint(0, 256, (P, h, w, 3)).astype(np.uint8)
    src = torch.from_numpy(base).cuda()[torch.arange(n, device="cuda") % P]
    out = native.resize_frames(src, size, box=box, rect=rect, fill=FC.FILL)
    _check_periodic(out, FM.fit(base, box, size, rect, FC.FILL))
    del out, src
    torch.cuda.empty_cache()


@pytest.mark.parametrize("h,w,size", [(37, 53, (24, 40)), (480, 640, (192, 280)), (301, 2, (24, 5)), (24, 40, (24, 40)),
                                      (37, 53, (37, 20)), (37, 53, (20, 53))])
def test_full_frame_geometry_is_the_plain_resize(native, h, w, size):
    """box = the whole frame, rect = the whole destination: bit for bit iiv_resize_frames / iiv_resize_frames_yuv420"""
    import torch
    src = np.random.RandomState(h + w).randint(0, 256, (2, h, w, 3)).astype(np.uint8)
    box, rect = (0, 0, w, h), (0, 0, size[1], size[0])
    plain = native.resize_frames(torch.from_numpy(src).cuda(), size).cpu().numpy()
    _same(fit_rgb(native, src, box, size, rect, fill=(9, 8, 7)), plain)
    planes = yuv_model.random_planes(2, h, w, h * w)
    for layout in LAYOUTS:
        plain = native.resize_frames_yuv420(*_device_planes(*planes, layout), size=size).cpu().numpy()
        _same(fit_yuv(native, planes, layout, box, size, rect, fill=(9, 8, 7)), plain)


@pytest.mark.parametrize("kind", ("rgb",) + LAYOUTS)
def test_random_geometries(native, kind):
    """a dozen seeded random geometries a source kind: fractional and whole-pixel boxes, boxes spanning an axis"""
    rng = np.random.RandomState({"rgb": 1, "i420": 2, "nv12": 3}[kind])
    for i in range(12):
        h, w = (int(v) for v in rng.randint(1, 70, 2))
        size = tuple(int(v) for v in rng.randint(1, 48, 2))
        box, rect = FC.random_geometry(rng, h, w, *size)
        if kind == "rgb":
            src = rng.randint(0, 256, (1, h, w, 3)).astype(np.uint8)
            got = fit_rgb(native, src, box, size, rect, lead=16 + i % 4)
        else:
            planes = yuv_model.random_planes(1, h, w, int(rng.randint(1 << 30)))
            src = yuv_model.to_rgb(*planes)
            got = fit_yuv(native, planes, kind, box, size, rect, lead=16 + i % 4)
        exp = FM.fit(src, box, size, rect, FC.FILL)
        assert np.array_equal(got, exp), "geometry %d: %dx%d box %s -> %s rect %s" % (i, h, w, box, size, rect)


@pytest.mark.parametrize("fit", ("letterbox", "crop"))
@pytest.mark.parametrize("mono", (False, True))
def test_frame_grabber_fit(native, fit, mono):
    """ArrayFrameGrabber(fit=...): the memory maps of RGB and (y, u, v) sources equal the ingest of the model's fitted frames,
    in colour (280 wide) and mono (560 dots)"""
    import frame_grabber as FG
    from palette import Palette
    from video_mode import VideoMode
    palette = Palette.MONO if mono else Palette.NTSC
    h, w, fill = 54, 128, (40, 90, 200)
    rgb = np.random.RandomState(81).randint(0, 256, (2, h, w, 3)).astype(np.uint8)
    planes = yuv_model.random_planes(2, h, w, 82)
    for source, frames in ((rgb, rgb), (planes, yuv_model.to_rgb(*planes))):
        g = FG.ArrayFrameGrabber(source, VideoMode.DHGR, palette=palette, resize=True, fit=fit, fill=fill)
        H, W = g.frame_size
        assert W == (560 if mono else 280)
        box, rect = FM.fit_geometry(h, w, H, W, fit)
        assert (box, rect) != FM.fit_geometry(h, w, H, W, "stretch")
        fitted = FM.fit(frames, box, (H, W), rect, fill)
        assert np.array_equal(g.ingest_frames().cpu().numpy(), fitted)
        ref = FG.ArrayFrameGrabber(fitted, VideoMode.DHGR, palette=palette)
        for a, b in zip(g.memory_maps(), ref.memory_maps()):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_on_a_busy_side_stream(native):
    """one call of each entry point on a non-blocking side stream behind a sleeping kernel (tests/stream_probe.py): every
    launch, the fill included, and the scratch are on the caller's stream, and box, rect and matrix are read before the return"""
    import ctypes
    L = native.lib()
    rng = np.random.default_rng(6)
    n, h, w, size = 2, 37, 53, (24, 40)
    box, rect = (5.25, 3.5, 50.75, 33.0), (3, 2, 31, 19)
    fill = FC.FILL[0] | FC.FILL[1] << 8 | FC.FILL[2] << 16
    dp = lambda t: ctypes.c_void_p(t.data_ptr())
    real = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    p = Probe()
    src = p.input(real, rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8))
    dst = p.output((n,) + size + (3,))
    h_box = p.host(np.array(box, np.float32), np.array((0, 0, w, h), np.float32))
    h_rect = p.host(np.array(rect, np.int32), np.array((0, 0, size[1], size[0]), np.int32))

    def call(st):
        ok(native, L.iiv_resize_frames_fit(n, h, w, dp(src), h * w * 3, w * 3, native.hptr(h_box), size[0], size[1],
                                           native.hptr(h_rect), fill, dp(dst), st))
    call(native.stream_ptr())   # the first use of a geometry uploads its tables
    p.run(call)
    _same(dst.cpu().numpy(), FM.fit(real, box, size, rect, FC.FILL))

    y, u, v = yuv_model.random_planes(n, h, w, 7)
    y2, u2, v2 = yuv_model.random_planes(n, h, w, 8)
    p = Probe()
    d_y, d_u, d_v = p.input(y, y2), p.input(u, u2), p.input(v, v2)
    dst = p.output((n,) + size + (3,))
    h_box = p.host(np.array(box, np.float32), np.array((0, 0, w, h), np.float32))
    h_rect = p.host(np.array(rect, np.int32), np.array((0, 0, size[1], size[0]), np.int32))
    m = p.host(native.yuv_matrix("bt601"), native.yuv_matrix("jpeg"))
    ch, cw = (h + 1) // 2, (w + 1) // 2

    def call_yuv(st):
        ok(native, L.iiv_resize_frames_yuv420_fit(n, h, w, dp(d_y), h * w, w, dp(d_u), dp(d_v), ch * cw, cw, 1, native.hptr(m),
                                                  native.hptr(h_box), size[0], size[1], native.hptr(h_rect), fill, dp(dst), st))
    call_yuv(native.stream_ptr())
    p.run(call_yuv)
    _same(dst.cpu().numpy(), FM.fit(yuv_model.to_rgb(y, u, v), box, size, rect, FC.FILL))
