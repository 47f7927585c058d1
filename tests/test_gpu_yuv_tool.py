"""GPU: tools/transcode_clip.py --yuv -- raw 4:2:0 frames as `ffmpeg -f rawvideo` writes them -> the .a2m bytes that --frames
writes on the model's RGB of the same planes (tests/yuv_model.py): the conversion inside the device resize changes nothing
behind it.  Once in DHGR with yuv420p, once in HGR with nv12 and BT.709; a file that is not a whole number of frames is refused."""
import os
import subprocess
import sys

import numpy as np
import pytest

import yuv_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "transcode_clip.py")
N, H, W = 6, 48, 64


def _clip():
    """six 64x48 frames: a luma ramp that drifts, two chroma gradients, some noise"""
    rng = np.random.RandomState(11)
    f, y, x = np.mgrid[0:N, 0:H, 0:W]
    luma = np.clip(16 + (x * 3 + y + 5 * f) % 220 + rng.randint(-6, 7, (N, H, W)), 0, 255).astype(np.uint8)
    f, y, x = np.mgrid[0:N, 0:H // 2, 0:W // 2]
    return luma, ((x * 8 + 3 * f) % 256).astype(np.uint8), ((y * 10 + 7 * f + 40) % 256).astype(np.uint8)


def _raw_bytes(y, u, v, pix_fmt):
    frames = []
    for i in range(N):
        chroma = np.stack([u[i], v[i]], axis=-1).tobytes() if pix_fmt == "nv12" else u[i].tobytes() + v[i].tobytes()
        frames.append(y[i].tobytes() + chroma)
    return b"".join(frames)


def _run(args):
    return subprocess.run([sys.executable, TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("mode,pix_fmt,matrix", [("DHGR", "yuv420p", None), ("HGR", "nv12", "bt709")])
def test_yuv_file_gives_the_bytes_of_its_rgb_frames(tmp_path, mode, pix_fmt, matrix):
    y, u, v = _clip()
    (tmp_path / "clip.yuv").write_bytes(_raw_bytes(y, u, v, pix_fmt))
    np.save(tmp_path / "clip.npy", yuv_model.to_rgb(y, u, v, matrix or "bt601"))
    common = ["--mode", mode, "--seed", "5", "--tick", "20"]
    r = _run(["--yuv", tmp_path / "clip.yuv", "--size", "%dx%d" % (W, H), "--out", tmp_path / "yuv.a2m"] + common
             + (["--pix-fmt", pix_fmt] if pix_fmt != "yuv420p" else []) + (["--yuv-matrix", matrix] if matrix else []))
    assert r.returncode == 0, r.stderr
    r = _run(["--frames", tmp_path / "clip.npy", "--out", tmp_path / "rgb.a2m"] + common)
    assert r.returncode == 0, r.stderr
    got, exp = (tmp_path / "yuv.a2m").read_bytes(), (tmp_path / "rgb.a2m").read_bytes()
    assert len(got) > 0 and got == exp


def test_a_truncated_file_is_refused(tmp_path):
    y, u, v = _clip()
    (tmp_path / "short.yuv").write_bytes(_raw_bytes(y, u, v, "yuv420p")[:-100])
    r = _run(["--yuv", tmp_path / "short.yuv", "--size", "%dx%d" % (W, H), "--out", tmp_path / "short.a2m"])
    assert r.returncode != 0 and "not a whole number" in r.stderr and not (tmp_path / "short.a2m").exists()
    r = _run(["--yuv", tmp_path / "short.yuv", "--out", tmp_path / "short.a2m"])           # --yuv without --size
    assert r.returncode != 0 and "--size" in r.stderr
