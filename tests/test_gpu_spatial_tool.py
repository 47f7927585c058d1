"""GPU: the command-line side of the spatial filter.  tools/transcode_clip.py without --denoise, --sharpen and --blur writes the .a2m
bytes an all-zero gain writes and the bytes of the same frames handed over as --frames (no stage in between); with the three flags
it writes the bytes of the same tool run on --frames that the model (tests/spatial_model.py) filtered beforehand, alone and together
with --levels and --temporal, with --yuv and --fit, and with --palette MONO.  One run goes through the command line in a process of
its own; the others call the tool's main() with the same argument lists in this process, which spares an interpreter, a library and a
device start each."""
import os
import subprocess
import sys

import numpy as np
import pytest

import levels_model
import spatial_cases as SC
import spatial_model as M
import temporal_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "transcode_clip.py")] + [str(x) for x in args], capture_output=True,
                         text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def _main(*args):
    """the tool's main() on an argument list, here"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import transcode_clip
    saved = sys.argv
    sys.argv = ["transcode_clip.py"] + [str(x) for x in args]
    try:
        transcode_clip.main()
    finally:
        sys.argv = saved


def _taps(sigma):
    import frame_grabber
    return frame_grabber.filter_taps(sigma)


def test_the_tool_filters_as_the_model_does(native, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import transcode_clip
    n, noise, seed = 3, 3, 11
    common = ["--seed", seed, "--dither", 32]
    card = transcode_clip.add_noise(transcode_clip.test_card(n), noise, seed)
    plain, zero = tmp_path / "plain.a2m", tmp_path / "zero.a2m"
    _main("--synthetic", n, "--synthetic-noise", noise, "--out", plain, *common)
    _main("--synthetic", n, "--synthetic-noise", noise, "--sharpen", "0", "--out", zero, *common)
    assert plain.read_bytes() == zero.read_bytes()        # a zero gain through the kernel: the bytes of no stage at all

    # the three flags: --blur 1.0,0.8 --denoise 4,12 --sharpen 384,16
    gain = SC.gain_table(denoise=(4, 12), sharpen=(384, 16))
    filtered = M.filter_frames(card, _taps(1.0), _taps(0.8), gain)
    np.save(tmp_path / "filtered.npy", filtered)
    by_tool, by_model = tmp_path / "tool.a2m", tmp_path / "model.a2m"
    _run("--synthetic", n, "--synthetic-noise", noise, "--blur", "1.0,0.8", "--denoise", "4,12", "--sharpen", "384,16", "--out", by_tool, *common)
    _main("--frames", tmp_path / "filtered.npy", "--out", by_model, *common)
    assert by_tool.read_bytes() == by_model.read_bytes() and by_tool.read_bytes() != plain.read_bytes()

    # the defaults: --denoise alone is the binomial blur; --sharpen AMOUNT alone has threshold 0, beside --denoise its HI
    for flags, kw in ((["--sharpen", "256"], dict(sharpen=(256, 0))),
                      (["--denoise", "3,9", "--sharpen", "300"], dict(denoise=(3, 9), sharpen=(300, 9)))):
        np.save(tmp_path / "f.npy", M.filter_frames(card, SC.BINOMIAL_TAPS, SC.BINOMIAL_TAPS, SC.gain_table(**kw)))
        _main("--synthetic", n, "--synthetic-noise", noise, *flags, "--out", by_tool, *common)
        _main("--frames", tmp_path / "f.npy", "--out", by_model, *common)
        assert by_tool.read_bytes() == by_model.read_bytes(), flags

    # with --levels and --temporal: levels, then the filter, then the hold
    lut = levels_model.levels_lut(20, 230)
    chain = temporal_model.hold(M.filter_frames(levels_model.apply(card, lut), SC.BINOMIAL_TAPS, SC.BINOMIAL_TAPS,
                                                SC.gain_table(denoise=(4, 12))), 6, 6)[0]
    np.save(tmp_path / "chain.npy", chain)
    _main("--synthetic", n, "--synthetic-noise", noise, "--levels", "20,230", "--denoise", "4,12", "--temporal", "6,6", "--out", by_tool, *common)
    _main("--frames", tmp_path / "chain.npy", "--out", by_model, *common)
    assert by_tool.read_bytes() == by_model.read_bytes()


def test_with_yuv_fit_and_mono(native, tmp_path):
    """the flags beside --yuv with --fit, and beside --palette MONO: the bytes of a grabber that filters, written by the tool's own
    path on the frames the grabber's model chain gives"""
    import frame_grabber
    from video_mode import VideoMode
    rng = np.random.default_rng(1695)
    n, h, w = 2, 90, 160
    raw = np.concatenate([np.clip(16 + np.arange(w)[None, None, :] + rng.integers(-4, 5, (n, h, w)), 0, 255).astype(np.uint8).reshape(n, -1),
                          rng.integers(100, 156, (n, 2 * (h // 2) * (w // 2))).astype(np.uint8)], axis=1)
    raw.tofile(tmp_path / "clip.yuv")
    common = ["--seed", 5, "--dither", 32]
    y = raw[:, :h * w].reshape(n, h, w)
    u = raw[:, h * w:h * w + (h // 2) * (w // 2)].reshape(n, h // 2, w // 2)
    v = raw[:, h * w + (h // 2) * (w // 2):].reshape(n, h // 2, w // 2)
    fitted = frame_grabber.ArrayFrameGrabber((y, u, v), VideoMode.DHGR, resize=True, fit="letterbox").ingest_frames().cpu().numpy()
    np.save(tmp_path / "f.npy", M.filter_frames(fitted, SC.BINOMIAL_TAPS, SC.BINOMIAL_TAPS, SC.gain_table(denoise=(4, 12), sharpen=(200, 12))))
    a, b = tmp_path / "a.a2m", tmp_path / "b.a2m"
    _main("--yuv", tmp_path / "clip.yuv", "--size", "%dx%d" % (w, h), "--fit", "letterbox", "--denoise", "4,12", "--sharpen", "200", "--out", a, *common)
    _main("--frames", tmp_path / "f.npy", "--out", b, *common)
    assert a.read_bytes() == b.read_bytes()

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import transcode_clip
    card = transcode_clip.add_noise(transcode_clip.test_card(n, 560), 3, 5)
    np.save(tmp_path / "m.npy", M.filter_frames(card, _taps(1.5), _taps(1.5), SC.gain_table(sharpen=(256, 8))))
    mono = ["--palette", "MONO", "--dither", 40, "--seed", 5]
    _main("--synthetic", n, "--synthetic-noise", 3, "--blur", "1.5", "--sharpen", "256,8", "--out", a, *mono)
    _main("--frames", tmp_path / "m.npy", "--out", b, *mono)
    assert a.read_bytes() == b.read_bytes()


def test_bad_arguments_are_refused(tmp_path):
    for args in (["--denoise", "7,3"], ["--denoise", "4"], ["--denoise", "0,256"], ["--sharpen", "1025"], ["--sharpen", "256,300"],
                 ["--denoise", "4,12", "--sharpen", "256,11"], ["--blur", "-1"], ["--blur", "1,2,3"], ["--blur", "x"]):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "transcode_clip.py"), "--synthetic", "2", "--out", str(tmp_path / "x.a2m")]
                             + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and "--denoise" in out.stderr, out.stderr
