"""GPU: ArrayFrameGrabber(temporal=(lo, hi)) -- the hold behind the resize and in front of every conversion.  temporal=None is a
grabber built without the argument; batches, one call and a call out of order give the same frames, maps and counts, and those are
the model (tests/temporal_model.py) run on the plain grabber's ingest frames, then the converter; (y, u, v) sources, a letterbox and
Palette.MONO go the same way; and the full-hold clip's memory maps repeat frame 0, which the same clip's do not without the hold."""
import numpy as np
import pytest

import temporal_cases as TC
import temporal_model as M

pytestmark = pytest.mark.gpu

PAIR = (5, 20)


def _moving_clip(n=8, size=(192, 280), seed=1491):
    """a still picture under noise of -8..8 with a block that moves four pixels a frame: pixels are held, blended and passed"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (1,) + size + (3,))
    a = base + rng.integers(-8, 9, (n,) + size + (3,))
    for t in range(n):
        a[t, 40:90, 20 + 4 * t:80 + 4 * t] = (250, 30 * t, 10)
    return np.clip(a, 0, 255).astype(np.uint8)


def _maps(grab, first=0, count=None):
    main, aux = grab.memory_maps(first, count)
    return main.cpu().numpy(), (aux.cpu().numpy() if aux is not None else None)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1]))


def _model_then_converter(plain, pair, **convert):
    """the plain grabber's ingest frames through the model, then through a grabber that only converts"""
    import frame_grabber
    frames = plain.ingest_frames().cpu().numpy()
    held, _, counts = M.hold(frames, *pair)
    return held, counts, _maps(frame_grabber.ArrayFrameGrabber(held, plain.video_mode, plain.palette, **convert))


def test_none_is_a_grabber_without_the_argument(native):
    import frame_grabber
    from video_mode import VideoMode
    clip = _moving_clip(4)
    for dither in (32, "diffusion", "direct"):
        a = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, dither=dither)
        b = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, dither=dither, temporal=None)
        assert _same(_maps(a), _maps(b))
        assert np.array_equal(a.ingest_frames().cpu().numpy(), clip) and np.array_equal(b.ingest_frames(1, 2).cpu().numpy(), clip[1:3])
        with pytest.raises(ValueError):
            b.temporal_counts()
    # (0, 0) is the identity: the same bytes again, through the kernel
    z = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, temporal=(0, 0))
    assert _same(_maps(z), _maps(frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR)))
    for bad in ((3, 2), (0, 256), (-1, 0), (1,), "x"):
        with pytest.raises(ValueError):
            frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, temporal=bad)


@pytest.mark.parametrize("mode_name,dither", [("DHGR", 32), ("HGR", "diffusion"), ("DHGR", "atkinson"), ("DHGR", "direct")])
def test_batches_one_call_and_out_of_order_equal_the_model(native, mode_name, dither):
    import frame_grabber
    from video_mode import VideoMode
    mode, clip = VideoMode[mode_name], _moving_clip(8)
    held, counts, want = _model_then_converter(frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither), PAIR, dither=dither)
    assert counts[1:].min(axis=0).min() > 0                       # every frame holds, blends and passes pixels
    one = frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither, temporal=PAIR)
    assert _same(_maps(one), want) and np.array_equal(one.temporal_counts(), counts)
    assert np.array_equal(one.ingest_frames().cpu().numpy(), held)
    # batches of 3 over 8 frames, continued from the grabber's state
    g = frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither, temporal=PAIR, batch=3)
    parts = [_maps(g, first, min(3, 8 - first)) for first in range(0, 8, 3)]
    got = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]) if parts[0][1] is not None else None)
    assert _same(got, want) and np.array_equal(g.temporal_counts(), counts)
    # out of order: frames 5..7, then 2..4 (from frame 0 again, in batches of 3), then 5..6 (continued)
    for first, count in ((5, 3), (2, 3), (5, 2)):
        part = _maps(g, first, count)
        assert np.array_equal(part[0], want[0][first:first + count]), (first, count)
        assert part[1] is None or np.array_equal(part[1], want[1][first:first + count]), (first, count)
        assert np.array_equal(g.temporal_counts(), counts[:first + count]), (first, count)
    # frames() walks the clip in batches and yields the same maps
    mains = np.stack([m.page_offset for m, _ in frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither, temporal=PAIR, batch=3).frames()])
    assert np.array_equal(mains, want[0])


def test_yuv_source(native):
    import frame_grabber
    from video_mode import VideoMode
    rng = np.random.default_rng(1492)
    n, h, w = 5, 96, 128
    y = np.clip(rng.integers(16, 236, (1, h, w)) + rng.integers(-4, 5, (n, h, w)), 0, 255).astype(np.uint8)
    u = np.clip(rng.integers(16, 241, (1, h // 2, w // 2)) + rng.integers(-3, 4, (n, h // 2, w // 2)), 0, 255).astype(np.uint8)
    v = np.clip(rng.integers(16, 241, (1, h // 2, w // 2)) + rng.integers(-3, 4, (n, h // 2, w // 2)), 0, 255).astype(np.uint8)
    y[2:, 30:60, 40:90] = 200
    plain = frame_grabber.ArrayFrameGrabber((y, u, v), VideoMode.DHGR, resize=True, yuv_matrix="bt709")
    held, counts, want = _model_then_converter(plain, PAIR)
    g = frame_grabber.ArrayFrameGrabber((y, u, v), VideoMode.DHGR, resize=True, yuv_matrix="bt709", temporal=PAIR, batch=2)
    assert _same(_maps(g), want) and np.array_equal(g.temporal_counts(), counts)
    assert counts[1:, 0].min() > 0 and counts[2, 2] > 0 and not _same(want, _maps(plain))


def test_letterbox(native):
    import frame_grabber
    from video_mode import VideoMode
    clip = _moving_clip(5, size=(90, 240), seed=1493)
    kw = dict(resize=True, fit="letterbox", fill=(10, 20, 30))
    plain = frame_grabber.ArrayFrameGrabber(clip, VideoMode.HGR, **kw)
    held, counts, want = _model_then_converter(plain, PAIR)
    g = frame_grabber.ArrayFrameGrabber(clip, VideoMode.HGR, temporal=PAIR, **kw)
    assert _same(_maps(g), want) and np.array_equal(g.temporal_counts(), counts)
    assert (held[:, 0, 0] == (10, 20, 30)).all() and not _same(want, _maps(plain))     # the bars are held from frame 1 on


def test_mono_palette(native):
    import frame_grabber
    from palette import Palette
    from video_mode import VideoMode
    clip = _moving_clip(4, size=(192, 560), seed=1494)
    plain = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, Palette.MONO, dither=40)
    held, counts, want = _model_then_converter(plain, PAIR, dither=40)
    g = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, Palette.MONO, dither=40, temporal=PAIR)
    assert _same(_maps(g), want) and np.array_equal(g.temporal_counts(), counts) and counts.sum(axis=1).tolist() == [192 * 560] * 4
    assert not _same(want, _maps(plain))


def test_full_hold_repeats_frame_zero(native):
    """the clip of tests/test_temporal_model.py: with the hold every frame's memory maps are frame 0's, without it they are not"""
    import frame_grabber
    from video_mode import VideoMode
    clip = TC.still_clip()
    main, aux = _maps(frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, dither=32, temporal=TC.HOLD_PAIR, batch=3))
    assert (main == main[:1]).all() and (aux == aux[:1]).all()
    plain_main, plain_aux = _maps(frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, dither=32))
    assert np.array_equal(plain_main[0], main[0]) and np.array_equal(plain_aux[0], aux[0])
    for t in range(1, TC.HOLD_FRAMES):
        assert (plain_main[t] != plain_main[0]).any() and (plain_aux[t] != plain_aux[t - 1]).any(), t
