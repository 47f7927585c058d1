"""GPU: ArrayFrameGrabber(levels=Levels(...)) -- the levels behind the resize and in front of the temporal hold and of every
conversion.  levels=None is a grabber built without the argument; batches, one call and a call out of order give the same frames
and maps, and those are the model (tests/levels_model.py) run on the plain grabber's ingest frames, then the converter; (y, u, v)
sources, a letterbox, temporal= and Palette.MONO go the same way; auto takes its points from the histogram of the first auto_frames
frames after the resize, per channel if asked, once."""
import numpy as np
import pytest

import levels_model as M
import temporal_model

pytestmark = pytest.mark.gpu


def _squeezed_clip(n=6, size=(192, 280), seed=1591, lo=40, hi=190):
    """a two-axis gradient with a moving block under a little noise, squeezed into lo..hi; the red channel a little narrower"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size[0], 0:size[1]]
    base = np.stack([(x * 255) // (size[1] - 1), (y * 255) // (size[0] - 1), ((x + y) * 255) // (size[0] + size[1] - 2)], axis=-1)
    a = base[None] + rng.integers(-3, 4, (n,) + base.shape)
    for t in range(n):
        a[t, 40:90, 20 + 4 * t:80 + 4 * t] = (250, 30 * t, 10)
    a = np.clip(a, 0, 255) * (hi - lo) // 255 + lo
    a[..., 0] = (a[..., 0] - lo) * 3 // 4 + lo + 10
    return a.astype(np.uint8)


def _maps(grab, first=0, count=None):
    main, aux = grab.memory_maps(first, count)
    return main.cpu().numpy(), (aux.cpu().numpy() if aux is not None else None)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1]))


def _model_tables(frames, lv, n_auto=None):
    """(lut (3, 256), matrix) of a Levels on the frames the plain grabber hands out, by the model"""
    points = [(lv.black, lv.white)] * 3
    if lv.auto is not None:
        hist = M.histogram(frames[:n_auto].reshape(-1, frames.shape[1] * frames.shape[2], 3)).astype(np.int64).sum(axis=0)
        points = [M.auto(hist[c], *lv.auto) for c in range(3)] if lv.per_channel else [M.auto(hist[3], *lv.auto)] * 3
    return points, np.stack([M.levels_lut(b, w, lv.gamma, lv.brightness, lv.contrast) for b, w in points]), M.saturation_matrix(lv.s256)


def _model_then_converter(plain, lv, n_auto=None, temporal=None, **convert):
    import frame_grabber
    frames = plain.ingest_frames().cpu().numpy()
    points, lut, m = _model_tables(frames, lv, n_auto)
    levelled = M.apply(frames, lut, m)
    if temporal is not None:
        levelled = temporal_model.hold(levelled, *temporal)[0]
    return points, levelled, _maps(frame_grabber.ArrayFrameGrabber(levelled, plain.video_mode, plain.palette, **convert))


def test_none_is_a_grabber_without_the_argument(native):
    import frame_grabber
    from video_mode import VideoMode
    clip = _squeezed_clip(4)
    for dither in (32, "diffusion", "direct"):
        a = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, dither=dither)
        b = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, dither=dither, levels=None)
        assert _same(_maps(a), _maps(b)) and np.array_equal(b.ingest_frames(1, 2).cpu().numpy(), clip[1:3])
        with pytest.raises(ValueError):
            b.levels_report()
    # the neutral Levels is the identity: the same bytes again, through the kernel
    z = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, levels=frame_grabber.Levels())
    assert _same(_maps(z), _maps(frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR)))
    r = z.levels_report()
    assert (r["black"], r["white"]) == (0, 255) and (r["lut"] == M.IDENTITY_LUT).all() and np.array_equal(r["matrix"], M.IDENTITY_MATRIX)
    for bad in ((0, 255), "auto", dict(black=3)):
        with pytest.raises(ValueError):
            frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, levels=bad)


@pytest.mark.parametrize("mode_name,dither", [("DHGR", 32), ("HGR", "diffusion"), ("DHGR", "direct")])
def test_batches_one_call_and_out_of_order_equal_the_model(native, mode_name, dither):
    import frame_grabber
    from video_mode import VideoMode
    mode, clip = VideoMode[mode_name], _squeezed_clip(6)
    lv = frame_grabber.Levels(black=40, white=190, gamma=1.3, brightness=4, contrast=1.1, saturation=1.5)
    _, levelled, want = _model_then_converter(frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither), lv, dither=dither)
    one = frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither, levels=lv)
    assert _same(_maps(one), want) and np.array_equal(one.ingest_frames().cpu().numpy(), levelled)
    assert not _same(want, _maps(frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither)))
    g = frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither, levels=lv, batch=4)
    parts = [_maps(g, first, min(4, 6 - first)) for first in range(0, 6, 4)]
    got = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]) if parts[0][1] is not None else None)
    assert _same(got, want)
    for first, count in ((4, 2), (1, 3), (0, 1)):
        part = _maps(g, first, count)
        assert np.array_equal(part[0], want[0][first:first + count]), (first, count)
        assert part[1] is None or np.array_equal(part[1], want[1][first:first + count]), (first, count)
    mains = np.stack([mm.page_offset for mm, _ in frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither, levels=lv, batch=4).frames()])
    assert np.array_equal(mains, want[0])


@pytest.mark.parametrize("per_channel,auto_frames", [(False, None), (False, 2), (True, None), (True, 3)])
def test_auto_takes_its_points_once_from_the_first_frames(native, per_channel, auto_frames):
    import frame_grabber
    from video_mode import VideoMode
    clip = _squeezed_clip(6)
    clip[4:, 100:120, 100:140] = (20, 25, 30)         # beyond any auto_frames: 1600 pixels at each end widen the whole clip's range
    clip[4:, 130:150, 100:140] = (215, 220, 225)      # (k is at most 967 of its 322 560 pixels), not the first frames'
    lv = frame_grabber.Levels(auto=(2000, 3000), per_channel=per_channel, auto_frames=auto_frames, gamma=1.2)
    plain = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR)
    points, levelled, want = _model_then_converter(plain, lv, auto_frames)
    # out of order first: frames 4..5 are levelled with points from frames 0 .. auto_frames - 1, found two frames at a time
    g = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, levels=lv, batch=2)
    assert np.array_equal(g.ingest_frames(4, 2).cpu().numpy(), levelled[4:])
    r = g.levels_report()
    if per_channel:
        assert list(zip(r["black"], r["white"])) == points and len(set(points)) > 1
    else:
        assert (r["black"], r["white"]) == points[0]
    assert points[0] != (0, 255) and r["auto"] == [2000, 3000] and r["auto_frames"] == auto_frames
    assert _same(_maps(g), want)
    whole = _model_tables(plain.ingest_frames().cpu().numpy(), lv, None)[0]
    assert (whole != points) == (auto_frames is not None)        # the late patch moves the whole clip's points only
    one = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, levels=lv)
    assert _same(_maps(one), want)


def test_yuv_source_with_letterbox_and_temporal(native):
    import frame_grabber
    from video_mode import VideoMode
    rng = np.random.default_rng(1592)
    n, h, w = 5, 90, 240
    y = np.clip(rng.integers(40, 180, (1, h, w)) + rng.integers(-4, 5, (n, h, w)), 0, 255).astype(np.uint8)
    u = np.clip(rng.integers(100, 156, (1, h // 2, w // 2)) + rng.integers(-3, 4, (n, h // 2, w // 2)), 0, 255).astype(np.uint8)
    v = np.clip(rng.integers(100, 156, (1, h // 2, w // 2)) + rng.integers(-3, 4, (n, h // 2, w // 2)), 0, 255).astype(np.uint8)
    y[2:, 30:60, 40:90] = 170
    kw = dict(resize=True, yuv_matrix="bt709", fit="letterbox", fill=(60, 60, 60))
    pair = (5, 20)
    lv = frame_grabber.Levels(auto=True, saturation=1.25)
    plain = frame_grabber.ArrayFrameGrabber((y, u, v), VideoMode.HGR, **kw)
    points, levelled, want = _model_then_converter(plain, lv, temporal=pair)
    g = frame_grabber.ArrayFrameGrabber((y, u, v), VideoMode.HGR, temporal=pair, levels=lv, batch=2, **kw)
    assert _same(_maps(g), want) and np.array_equal(g.ingest_frames().cpu().numpy(), levelled)
    assert points[0] != (0, 255) and (g.levels_report()["black"], g.levels_report()["white"]) == points[0]
    # the hold's thresholds are in the levelled values: holding first and levelling afterwards gives other bytes
    frames = plain.ingest_frames().cpu().numpy()
    _, lut, m = _model_tables(frames, lv)
    assert not np.array_equal(M.apply(temporal_model.hold(frames, *pair)[0], lut, m), levelled)
    assert not _same(want, _maps(frame_grabber.ArrayFrameGrabber((y, u, v), VideoMode.HGR, temporal=pair, **kw)))


def test_mono_palette(native):
    import frame_grabber
    from palette import Palette
    from video_mode import VideoMode
    clip = _squeezed_clip(3, size=(192, 560), seed=1594, lo=85, hi=170)       # a third of the range: the 1-bit dither's worst case
    lv = frame_grabber.Levels(auto=True)
    plain = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, Palette.MONO, dither=40)
    points, levelled, want = _model_then_converter(plain, lv, dither=40)
    g = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, Palette.MONO, dither=40, levels=lv)
    assert _same(_maps(g), want) and not _same(want, _maps(plain))
    assert 85 <= points[0][0] < points[0][1] <= 180 and int(levelled.min()) == 0 and int(levelled.max()) == 255
