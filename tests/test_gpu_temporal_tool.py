"""GPU: the command-line side of the temporal hold.  tools/transcode_clip.py --temporal 0,0 writes the .a2m bytes of a run without
the flag; --synthetic 6 --synthetic-noise 3 --temporal 6,6 writes the bytes of the same tool run on --frames that the model
(tests/temporal_model.py) filtered beforehand; and --quality carries the three counts per frame with --temporal and nothing new
without it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import temporal_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "transcode_clip.py")] + [str(x) for x in args], capture_output=True,
                         text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def test_the_tool_holds_as_the_model_does(native, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import transcode_clip
    n, noise, seed = 6, 3, 11
    common = ["--seed", seed, "--dither", 32]
    plain, zero = tmp_path / "plain.a2m", tmp_path / "zero.a2m"
    _run("--synthetic", n, "--synthetic-noise", noise, "--out", plain, "--quality", tmp_path / "plain.json", *common)
    _run("--synthetic", n, "--synthetic-noise", noise, "--temporal", "0,0", "--out", zero, *common)
    assert plain.read_bytes() == zero.read_bytes()

    card = transcode_clip.add_noise(transcode_clip.test_card(n), noise, seed)
    assert np.array_equal(transcode_clip.add_noise(transcode_clip.test_card(n), 0, seed), transcode_clip.test_card(n))
    assert int(np.abs(card.astype(int) - transcode_clip.test_card(n)).max()) == noise
    held, _, counts = M.hold(card, 6, 6)
    np.save(tmp_path / "held.npy", held)
    by_tool, by_model = tmp_path / "tool.a2m", tmp_path / "model.a2m"
    _run("--synthetic", n, "--synthetic-noise", noise, "--temporal", "6,6", "--out", by_tool, "--quality", tmp_path / "tool.json", *common)
    _run("--frames", tmp_path / "held.npy", "--out", by_model, *common)
    assert by_tool.read_bytes() == by_model.read_bytes()
    assert by_tool.read_bytes() != plain.read_bytes()
    # the counts: in the JSON with --temporal, the model's; nothing new without
    with open(tmp_path / "tool.json") as f:
        q = json.load(f)
    assert q["temporal"] == {"lo": 6, "hi": 6, "counts": ["held", "blended", "passed"]}
    assert [e["temporal"] for e in q["frames"]] == counts.tolist()
    assert counts[1:, 0].min() > 192 * 280 // 2 and counts[1:, 2].min() > 0        # most of the card is still, the bars' edges move
    with open(tmp_path / "plain.json") as f:
        p = json.load(f)
    assert "temporal" not in p and all("temporal" not in e for e in p["frames"]) and set(p) == set(q) - {"temporal"}


def test_bad_arguments_are_refused(tmp_path):
    for args in (["--synthetic", 2, "--temporal", "7,3"], ["--synthetic", 2, "--temporal", "4"], ["--synthetic", 2, "--temporal", "0,256"],
                 ["--synthetic", 2, "--synthetic-noise", -1], ["--frames", "x.npy", "--synthetic-noise", 3]):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "transcode_clip.py"), "--out", str(tmp_path / "x.a2m")]
                             + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and ("--temporal" in out.stderr or "--synthetic-noise" in out.stderr), out.stderr
