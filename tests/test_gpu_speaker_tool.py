"""GPU: the command-line side of the speaker preview.  tools/play_a2m.py --audio on a stream tools/transcode_clip.py --synthetic
wrote gives a .wav whose frames are A2mReader.speaker_pcm's samples at audio.speaker_rate's rate; transcode_clip.py
--preview-audio writes the same samples; and the .a2m bytes do not depend on the flag."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import a2m_model
import speaker_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wav(path):
    with wave.open(str(path), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2"), w.getframerate()


def test_tools_write_the_readers_samples(native, tmp_path):
    import a2m
    import audio
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))

    def run(tool, *args):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)] + [str(x) for x in args], capture_output=True, text=True,
                             env=env, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        return out
    # a tick track of its own, so that the samples are not one pulse repeated
    t = np.arange(22050) / 44100.0
    pcm = np.clip(np.round(12000 * np.sin(2 * np.pi * 330.0 * t)), -32768, 32767).astype(np.int16)
    np.save(tmp_path / "pcm.npy", pcm)
    plain, flagged = tmp_path / "plain.a2m", tmp_path / "flagged.a2m"
    common = ["--synthetic", 3, "--pcm", tmp_path / "pcm.npy", "--rate", 44100]
    run("transcode_clip.py", *common, "--out", plain)
    run("transcode_clip.py", *common, "--out", flagged, "--preview-audio", tmp_path / "preview.wav")
    data = np.fromfile(plain, dtype=np.uint8)
    assert np.array_equal(data, np.fromfile(flagged, dtype=np.uint8))

    r = a2m.A2mReader(a2m.OpcodeAddresses.placeholder())
    try:
        want = r.speaker_pcm([data])[0].cpu().numpy()
        want_other = r.speaker_pcm([data], decim=64, order=2, gain=30000)[0].cpu().numpy()
    finally:
        r.close()
    addr = a2m.OpcodeAddresses.placeholder()
    _, _, ticks, _ = a2m_model.decode(data, addr.tick, addr.ack, addr.terminate)
    assert len(ticks) > 584 and len(set(ticks.tolist())) > 8          # past two ACKs, and a real tick track
    assert np.array_equal(want, M.pcm(ticks)[0])

    got, rate = _wav(tmp_path / "preview.wav")
    assert rate == audio.speaker_rate() == 44369 and np.array_equal(got, want)
    run("play_a2m.py", plain, "--audio", tmp_path / "played.wav")
    got, rate = _wav(tmp_path / "played.wav")
    assert rate == 44369 and np.array_equal(got, want)
    run("play_a2m.py", plain, "--audio", tmp_path / "other.wav", "--decim", 64, "--order", 2, "--gain", 30000, "--clock", 1000000)
    got, rate = _wav(tmp_path / "other.wav")
    assert rate == audio.speaker_rate(64, 1000000) == 15625 and np.array_equal(got, want_other)
    assert np.array_equal(np.fromfile(plain, dtype=np.uint8), data)
