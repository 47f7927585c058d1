"""GPU: csrc/iiv_resize.hip -- frames of any size -> 280x192 (frame_grabber.py:75,100) -- equals the tests' numpy model
(tests/resize_model.py, itself held to Pillow by tests/test_resize_host.py) byte for byte, and Pillow directly: through
the committed fixture tests/golden/g9_resize.npz always, and live when Pillow imports.  Then the strided input, the
stream contract, ArrayFrameGrabber(resize=True) and tools/transcode_clip.py on a 640x480 clip."""
import os
import subprocess
import sys

import numpy as np
import pytest

import resize_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXED, RANDOM = M.sizes()


def _frames(h, w, n, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)


def _device(native, a, size):
    import torch
    return native.resize_frames(torch.from_numpy(a).cuda(), size).cpu().numpy()


@pytest.mark.parametrize("h,w,H,W", FIXED)
def test_device_equals_model_fixed(native, h, w, H, W):
    a = _frames(h, w, 1 if h * w > 100000 else 3, h + 3 * w)
    assert np.array_equal(_device(native, a, (H, W)), M.resize(a, (H, W)))


def test_device_equals_model_random_pairs(native):
    for i, (h, w, H, W) in enumerate(RANDOM):
        a = _frames(h, w, 2, 1000 + i)
        assert np.array_equal(_device(native, a, (H, W)), M.resize(a, (H, W))), (h, w, H, W)


@pytest.mark.parametrize("h,w,n", [(2160, 3840, 2), (24, 8192, 2), (3, 8192, 1), (8192, 3, 1), (8192, 100, 1)])
def test_device_equals_model_large(native, h, w, n):
    a = _frames(h, w, n, 77)
    for size in ((192, 280),) + (((1024, 1024),) if h * w < 1 << 20 else ()):
        assert np.array_equal(_device(native, a, size), M.resize(a, size)), size


def test_device_equals_pillow(native, golden):
    g = golden.g9_resize
    i = 0
    while "src_%d" % i in g:
        src, dst = g["src_%d" % i], g["dst_%d" % i]
        assert np.array_equal(_device(native, src[None], dst.shape[:2])[0], dst), i
        i += 1
    assert i >= 6
    try:
        import PIL  # noqa: F401
    except ImportError:
        return   # the fixture above is Pillow's own output
    for (h, w, H, W) in FIXED[:6] + RANDOM[:20]:
        a = _frames(h, w, 1, h * w)
        assert np.array_equal(_device(native, a, (H, W)), M.pillow_resize(a, (H, W))), (h, w, H, W)


def test_strided_views_equal_their_contiguous_copies(native):
    import torch
    big = torch.from_numpy(_frames(500, 700, 3, 5)).cuda()
    views = [big[:, 10:490, 30:670],          # a crop: row stride 2100, offset not 4-byte aligned
             big[::2, 7:400, 1:640],          # every other frame, odd offset
             big[:, 3:4, 5:645],              # one row: only the horizontal pass
             big[:, 11:491, 33:34]]           # one column
    for v in views:
        for size in ((192, 280), (192, int(v.shape[2])), (int(v.shape[1]), 280)):
            got = native.resize_frames(v, size)
            exp = native.resize_frames(v.contiguous(), size)
            assert torch.equal(got, exp), (tuple(v.shape), size)
            assert np.array_equal(got.cpu().numpy(), M.resize(v.cpu().numpy(), size))
    with pytest.raises(ValueError):
        native.resize_frames(big[:, :, :, :2])
    with pytest.raises(ValueError):
        native.resize_frames(big.permute(0, 2, 1, 3))


def test_side_stream_and_no_host_synchronisation(native):
    import torch
    a = _frames(480, 640, 4, 9)
    src = torch.from_numpy(a).cuda()
    exp = M.resize(a, (192, 280))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out1 = native.resize_frames(src, (192, 280))      # (may be the first use of 640 -> 280 / 480 -> 192: uploads)
    side.synchronize()
    assert np.array_equal(out1.cpu().numpy(), exp)
    out2 = torch.zeros((4, 192, 280, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(200_000_000)                  # keeps the side stream busy for tens of milliseconds
        native.resize_frames(src, (192, 280), out=out2)
        busy = not side.query()                         # the call returned while the stream was still sleeping
    assert busy, "a second call with the same size pair synchronised the host"
    side.synchronize()
    assert np.array_equal(out2.cpu().numpy(), exp)


def test_frame_grabber_resizes_on_the_device(native):
    import frame_grabber
    import palette
    import video_mode
    a = _frames(480, 640, 3, 21)
    try:
        small = M.pillow_resize(a, (192, 280))
    except ImportError:
        small = M.resize(a, (192, 280))
    for vm, dither in ((video_mode.VideoMode.DHGR, 32), (video_mode.VideoMode.HGR, "diffusion")):
        got = frame_grabber.ArrayFrameGrabber(a, vm, palette.Palette.NTSC, dither=dither, resize=True, batch=2)
        exp = frame_grabber.ArrayFrameGrabber(small, vm, palette.Palette.NTSC, dither=dither)
        gm, ga = got.memory_maps()
        em, ea = exp.memory_maps()
        assert np.array_equal(gm.cpu().numpy(), em.cpu().numpy())
        assert (ga is None and ea is None) or np.array_equal(ga.cpu().numpy(), ea.cpu().numpy())
        for (m1, x1), (m2, x2) in zip(got.frames(), exp.frames()):   # the batched path (batch=2) too
            assert np.array_equal(m1.page_offset, m2.page_offset)
    with pytest.raises(ValueError):
        frame_grabber.ArrayFrameGrabber(a, video_mode.VideoMode.HGR)   # the default still wants 280x192


def test_transcode_clip_resizes_a_640x480_clip(tmp_path):
    a = _frames(480, 640, 4, 33)
    a[:, 100:300, 200:500] = (255, 40, 0)
    try:
        small = M.pillow_resize(a, (192, 280))
    except ImportError:
        small = M.resize(a, (192, 280))
    outs = []
    for name, clip in (("big", a), ("small", small)):
        np.save(tmp_path / (name + ".npy"), clip)
        out = tmp_path / (name + ".a2m")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "transcode_clip.py"), "--frames",
                            str(tmp_path / (name + ".npy")), "--out", str(out), "--seed", "3"],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        outs.append(out.read_bytes())
    assert len(outs[0]) > 0 and outs[0] == outs[1]
