"""GPU: the command-line side of picture levels.  tools/transcode_clip.py without the options writes the .a2m bytes it wrote before
(those of a run on --frames holding the same card); --synthetic-range 64,160 with --levels auto:LO,HI --gamma
--saturation writes the bytes of the same tool run on --frames that the model (tests/levels_model.py) levelled beforehand; and
--quality carries the picture_levels block with the options and nothing new without them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import levels_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "transcode_clip.py")


def _run(*args):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    out = subprocess.run([sys.executable, TOOL] + [str(x) for x in args], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def test_the_tool_levels_as_the_model_does(native, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import transcode_clip
    n, seed = 4, 11
    common = ["--seed", seed, "--dither", 32]
    card = transcode_clip.test_card(n)
    squeezed = transcode_clip.squeeze(card, 64, 160)
    assert squeezed.min() == 64 and squeezed.max() == 160 and transcode_clip.squeeze(card, 0, 255) is card
    assert np.array_equal(squeezed, ((card.astype(np.int64) * 192 + 255) // 510 + 64).astype(np.uint8))
    np.save(tmp_path / "card.npy", card)
    # without the options: the bytes of before
    plain, frames = tmp_path / "plain.a2m", tmp_path / "frames.a2m"
    _run("--synthetic", n, "--out", plain, "--quality", tmp_path / "plain.json", *common)
    _run("--frames", tmp_path / "card.npy", "--out", frames, *common)
    assert plain.read_bytes() == frames.read_bytes()
    # --synthetic-range with --levels auto:LO,HI, --gamma and --saturation
    hist = M.histogram(squeezed.reshape(n, -1, 3)).astype(np.int64).sum(axis=0)
    black, white = M.auto(hist[3], 100000, 200000)
    assert 64 < black < white < 160 and (black, white) != M.auto(hist[3])
    np.save(tmp_path / "auto.npy", M.apply(squeezed, M.levels_lut(black, white, 1.8, 0, 1.0), M.saturation_matrix(384)))
    by_tool, by_model = tmp_path / "tool.a2m", tmp_path / "model.a2m"
    _run("--synthetic", n, "--synthetic-range", "64,160", "--levels", "auto:100000,200000", "--gamma", 1.8, "--saturation", 1.5, "--out", by_tool,
         "--quality", tmp_path / "tool.json", *common)
    _run("--frames", tmp_path / "auto.npy", "--out", by_model, *common)
    assert by_tool.read_bytes() == by_model.read_bytes() and by_tool.read_bytes() != plain.read_bytes()
    with open(tmp_path / "tool.json") as f:
        q = json.load(f)
    lv = q["picture_levels"]
    assert (lv["black"], lv["white"], lv["auto"], lv["per_channel"]) == (black, white, [100000, 200000], False)
    assert (lv["gamma"], lv["brightness"], lv["contrast"], lv["saturation"]) == (1.8, 0.0, 1.0, 1.5)
    assert np.array_equal(np.array(lv["lut"]), np.broadcast_to(M.levels_lut(black, white, 1.8, 0, 1.0), (3, 256)))
    assert lv["matrix"] == M.saturation_matrix(384).tolist()
    with open(tmp_path / "plain.json") as f:
        p = json.load(f)
    assert "picture_levels" not in p and set(p) == set(q) - {"picture_levels"}


def test_bad_arguments_are_refused(tmp_path):
    for args in (["--synthetic", 2, "--levels", "160,64"], ["--synthetic", 2, "--levels", "auto:1"], ["--synthetic", 2, "--levels", "auto:0,500001"],
                 ["--synthetic", 2, "--levels", "x"], ["--synthetic", 2, "--gamma", 0], ["--synthetic", 2, "--saturation", 5],
                 ["--synthetic", 2, "--contrast", -1], ["--synthetic", 2, "--synthetic-range", "160,64"],
                 ["--frames", "x.npy", "--synthetic-range", "64,160"]):
        out = subprocess.run([sys.executable, TOOL, "--out", str(tmp_path / "x.a2m")] + [str(a) for a in args], capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 2 and ("--levels" in out.stderr or "--gamma" in out.stderr or "--synthetic-range" in out.stderr), out.stderr
