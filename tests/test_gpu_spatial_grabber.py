"""GPU: ArrayFrameGrabber(spatial=Spatial(...)) -- the filter behind the levels and in front of the hold.  spatial=None is a grabber
built without the argument; batches, one call and a call out of order give the same frames and maps, and those are the model
(tests/spatial_model.py) run on the plain grabber's ingest frames, then the converter; (y, u, v) sources, a letterbox and Palette.MONO
go the same way; and with levels= and temporal= beside it the order is levels, then filter, then hold."""
import numpy as np
import pytest

import levels_model
import spatial_model as M
import temporal_model

pytestmark = pytest.mark.gpu

DENOISE, SHARPEN = (4, 12), (384, 16)


def _clip(n=5, size=(192, 280), seed=1691):
    """a soft picture under noise of -5..5 with a block that moves four pixels a frame: flat parts, noise and hard edges"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size[0], 0:size[1]]
    base = np.stack([(x * 255) // (size[1] - 1), (y * 255) // (size[0] - 1), 128 + 0 * x], axis=-1)
    a = base[None] + rng.integers(-5, 6, (n,) + size + (3,))
    for t in range(n):
        a[t, 40:90, 20 + 4 * t:80 + 4 * t] = (250, 30 * t, 10)
    return np.clip(a, 0, 255).astype(np.uint8)


def _spatial():
    import frame_grabber
    return frame_grabber.Spatial(blur=(1.0, 0.8), denoise=DENOISE, sharpen=SHARPEN)


def _maps(grab, first=0, count=None):
    main, aux = grab.memory_maps(first, count)
    return main.cpu().numpy(), (aux.cpu().numpy() if aux is not None else None)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1]))


def _model_then_converter(plain, spatial, **convert):
    """the plain grabber's ingest frames through the model, then through a grabber that only converts"""
    import frame_grabber
    frames = plain.ingest_frames().cpu().numpy()
    filtered = M.filter_frames(frames, spatial.taps_x, spatial.taps_y, spatial.gain)
    m = np.abs(frames.astype(int) - M.blur(frames, spatial.taps_x, spatial.taps_y)).max(axis=-1)
    assert (m <= DENOISE[0]).any() and ((m > DENOISE[0]) & (m <= DENOISE[1])).any() and (m > SHARPEN[1]).any()
    return filtered, _maps(frame_grabber.ArrayFrameGrabber(filtered, plain.video_mode, plain.palette, **convert))


def test_none_is_a_grabber_without_the_argument(native):
    import frame_grabber
    from video_mode import VideoMode
    clip = _clip(3)
    for dither in (32, "diffusion", "direct"):
        a = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, dither=dither)
        b = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, dither=dither, spatial=None)
        assert _same(_maps(a), _maps(b))
        assert np.array_equal(b.ingest_frames(1, 2).cpu().numpy(), clip[1:3])
    # an all-zero gain is the identity: the same bytes again, through the kernel
    z = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, spatial=frame_grabber.Spatial())
    assert _same(_maps(z), _maps(frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR)))
    for bad in ((4, 12), "x", 1):
        with pytest.raises(ValueError):
            frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, spatial=bad)


@pytest.mark.parametrize("mode_name,dither", [("DHGR", 32), ("HGR", "diffusion"), ("DHGR", "direct")])
def test_batches_one_call_and_out_of_order_equal_the_model(native, mode_name, dither):
    import frame_grabber
    from video_mode import VideoMode
    mode, clip, sp = VideoMode[mode_name], _clip(5), _spatial()
    plain = frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither)
    filtered, want = _model_then_converter(plain, sp, dither=dither)
    assert not _same(want, _maps(plain))
    one = frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither, spatial=sp)
    assert _same(_maps(one), want) and np.array_equal(one.ingest_frames().cpu().numpy(), filtered)
    g = frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither, spatial=sp, batch=2)
    parts = [_maps(g, first, min(2, 5 - first)) for first in range(0, 5, 2)]
    got = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]) if parts[0][1] is not None else None)
    assert _same(got, want)
    for first, count in ((3, 2), (1, 2), (4, 1)):
        part = _maps(g, first, count)
        assert np.array_equal(part[0], want[0][first:first + count]), (first, count)
        assert part[1] is None or np.array_equal(part[1], want[1][first:first + count]), (first, count)
    mains = np.stack([m.page_offset for m, _ in frame_grabber.ArrayFrameGrabber(clip, mode, dither=dither, spatial=sp, batch=2).frames()])
    assert np.array_equal(mains, want[0])


def test_yuv_source(native):
    import frame_grabber
    from video_mode import VideoMode
    rng = np.random.default_rng(1692)
    n, h, w = 3, 96, 128
    yy, xx = np.mgrid[0:h, 0:w]
    y = np.clip(16 + (xx * 219) // (w - 1) + rng.integers(-4, 5, (n, h, w)), 0, 255).astype(np.uint8)
    u = np.clip(rng.integers(100, 156, (1, h // 2, w // 2)) + rng.integers(-3, 4, (n, h // 2, w // 2)), 0, 255).astype(np.uint8)
    v = np.clip(rng.integers(100, 156, (1, h // 2, w // 2)) + rng.integers(-3, 4, (n, h // 2, w // 2)), 0, 255).astype(np.uint8)
    y[1:, 30:60, 40:90] = 200
    sp = _spatial()
    plain = frame_grabber.ArrayFrameGrabber((y, u, v), VideoMode.DHGR, resize=True, yuv_matrix="bt709")
    filtered, want = _model_then_converter(plain, sp)
    g = frame_grabber.ArrayFrameGrabber((y, u, v), VideoMode.DHGR, resize=True, yuv_matrix="bt709", spatial=sp, batch=2)
    assert _same(_maps(g), want) and not _same(want, _maps(plain))


def test_letterbox(native):
    import frame_grabber
    from video_mode import VideoMode
    clip = _clip(3, size=(90, 240), seed=1693)
    kw = dict(resize=True, fit="letterbox", fill=(10, 20, 30))
    sp = _spatial()
    plain = frame_grabber.ArrayFrameGrabber(clip, VideoMode.HGR, **kw)
    filtered, want = _model_then_converter(plain, sp)
    g = frame_grabber.ArrayFrameGrabber(clip, VideoMode.HGR, spatial=sp, **kw)
    assert _same(_maps(g), want) and not _same(want, _maps(plain))
    assert (filtered[:, 0, 0] == (10, 20, 30)).all()                  # the bars are flat: a fixed point


def test_mono_palette(native):
    import frame_grabber
    from palette import Palette
    from video_mode import VideoMode
    clip = _clip(3, size=(192, 560), seed=1694)
    sp = _spatial()
    plain = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, Palette.MONO, dither=40)
    filtered, want = _model_then_converter(plain, sp, dither=40)
    g = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, Palette.MONO, dither=40, spatial=sp)
    assert _same(_maps(g), want) and not _same(want, _maps(plain))
    assert filtered.shape == (3, 192, 560, 3)


def test_the_order_is_levels_then_filter_then_hold(native):
    import frame_grabber
    from video_mode import VideoMode
    clip, sp, pair = _clip(5), _spatial(), (5, 20)
    levels = frame_grabber.Levels(black=20, white=230, gamma=1.2, saturation=1.3)
    g = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, levels=levels, spatial=sp, temporal=pair, batch=2)
    got = np.concatenate([g.ingest_frames(first, min(2, 5 - first)).cpu().numpy() for first in range(0, 5, 2)])
    rep = g.levels_report()
    levelled = levels_model.apply(clip, rep["lut"], rep["matrix"].astype(np.int64))
    filtered = M.filter_frames(levelled, sp.taps_x, sp.taps_y, sp.gain)
    held, _, counts = temporal_model.hold(filtered, *pair)
    assert np.array_equal(got, held) and np.array_equal(g.temporal_counts(), counts)
    # every other order gives other bytes, so the comparison above tells them apart
    other = temporal_model.hold(levels_model.apply(M.filter_frames(clip, sp.taps_x, sp.taps_y, sp.gain), rep["lut"], rep["matrix"].astype(np.int64)), *pair)[0]
    assert (other != held).any()
    other = M.filter_frames(temporal_model.hold(levelled, *pair)[0], sp.taps_x, sp.taps_y, sp.gain)
    assert (other != held).any()
    # the pairs alone: levels then filter, filter then hold
    g = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, levels=levels, spatial=sp)
    assert np.array_equal(g.ingest_frames().cpu().numpy(), filtered)
    g = frame_grabber.ArrayFrameGrabber(clip, VideoMode.DHGR, spatial=sp, temporal=pair)
    assert np.array_equal(g.ingest_frames().cpu().numpy(), temporal_model.hold(M.filter_frames(clip, sp.taps_x, sp.taps_y, sp.gain), *pair)[0])
