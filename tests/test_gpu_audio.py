"""GPU: the audio track (csrc/iiv_audio.hip) against the tests' model of the reference (tests/audio_model.py, float64):
the resample of one block, the ticks of batches of streams, the normalisation, and transcode_clip.py end to end."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import audio_model as M
from audio_model import check_ticks as _check_ticks, signal as _signal   # (shared with tests/stage_fuzz.py)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(pcms):
    """list of int16 (n, ch) -> CUDA int16 (S, max n * ch), frame counts, channels"""
    import torch
    width = max(p.size for p in pcms)
    host = np.zeros((len(pcms), max(width, 1)), np.int16)
    for s, p in enumerate(pcms):
        host[s, :p.size] = p.reshape(-1)
    return torch.from_numpy(host).cuda(), [p.shape[0] for p in pcms], [p.shape[1] for p in pcms]


RESAMPLE_N = [1, 2, 3, 682, 683, 2047, 2048, 4097, 32768, 131072, 2622464]
RATES = [8000, 22050, 44100, 48000, 96000, 14700]


@pytest.mark.parametrize("rate", RATES)
def test_resample_one_block_equals_the_model(native, rate):
    pcms = [_signal("noise" if i % 2 else "chirp", n, 1 + i % 2, 10 + i) for i, n in enumerate(RESAMPLE_N)]
    pcm, nf, ch = _batch(pcms)
    y, lens = native.audio_resample(pcm, nf, ch, rate)
    y = y.cpu().numpy()
    for s, p in enumerate(pcms):
        want = M.decode(p.reshape(-1), p.shape[1], rate)
        assert lens[s] == len(want) == M.n_out(p.shape[0], rate)
        err = np.abs(y[s, :lens[s]] - want).max()
        assert err <= 1e-5 * np.abs(want).max(), "N=%d rate=%d: max error %g of max |y| %g" % (p.shape[0], rate, err, np.abs(want).max())


@pytest.mark.parametrize("block_frames", [131072, 2048, 3001])
def test_ticks_of_a_batch_equal_the_model(native, block_frames):
    import torch
    specs = [("sine", 300000, 2, 44100), ("chirp", 140001, 1, 44100), ("noise", 97, 2, 44100), ("loud", 262144, 2, 44100),
             ("noise", 50000, 1, 44100), ("sine", 131073, 2, 44100), ("noise", 2049, 2, 44100)]
    pcms = [_signal(k, n, c, i) for i, (k, n, c, _) in enumerate(specs)]
    pcm, nf, ch = _batch(pcms)
    norms = [M.normalization(p.reshape(-1), p.shape[1], 44100) for p in pcms]
    counts = [M.tick_count(n, 44100, block_frames=block_frames) for n in nf]
    out = torch.full((len(pcms), max(counts) + 64), 0xAB, dtype=torch.uint8, device="cuda")
    t, got_counts = native.audio_ticks(pcm, nf, ch, 44100, norms, block_frames=block_frames, out=out)
    assert t is out and list(got_counts) == counts
    host = out.cpu().numpy()
    for s, p in enumerate(pcms):
        want, v = M.ticks(p.reshape(-1), p.shape[1], 44100, norms[s], block_frames=block_frames)
        assert len(want) == counts[s]
        _check_ticks(host[s, :counts[s]], want, v)
        assert (host[s, counts[s]:] == 0xAB).all(), "bytes past the tick count were written"
        assert set(np.unique(host[s, :counts[s]])) <= set(range(4, 67, 2))


def test_ticks_other_rates_and_identity(native):
    pcms = [_signal("noise", 70000, 2, 1), _signal("sine", 40000, 1, 2), _signal("chirp", 5000, 2, 3)]
    for rate in (48000, 8000, 14700):
        pcm, nf, ch = _batch(pcms)
        norms = [3.1, 2.0, 1.7]
        t, counts = native.audio_ticks(pcm, nf, ch, rate, norms, block_frames=4096)
        host = t.cpu().numpy()
        for s, p in enumerate(pcms):
            want, v = M.ticks(p.reshape(-1), p.shape[1], rate, norms[s], block_frames=4096)
            assert counts[s] == len(want)
            _check_ticks(host[s, :counts[s]], want, v)


def test_normalization_equals_the_model(native):
    pcms = [_signal("noise", 3_000_000, 2, 5), _signal("sine", 300000, 1, 6), _signal("loud", 2_700_000, 1, 7),
            _signal("chirp", 1234, 2, 8)]
    for rate in (44100, 14700):
        pcm, nf, ch = _batch(pcms)
        got = native.audio_normalization(pcm, nf, ch, rate)
        for s, p in enumerate(pcms):
            want = M.normalization(p.reshape(-1), p.shape[1], rate)
            assert abs(got[s] - want) <= 1e-5 * abs(want), (s, rate, got[s], want)


def test_silent_prefix_refused(native):
    import audio
    import torch
    pcm = torch.zeros((1, 20000), dtype=torch.int16, device="cuda")
    assert np.isinf(native.audio_normalization(pcm, 10000, 2, 44100)[0])
    with pytest.raises(native.IIVError) as e:
        native.audio_ticks(pcm, 10000, 2, 44100, np.inf)
    assert e.value.code == native.ERR_INVALID
    for bad in (0.0, np.nan):
        with pytest.raises(native.IIVError):
            native.audio_ticks(pcm, 10000, 2, 44100, bad)
    with pytest.raises(native.IIVError):
        audio.ArrayAudio(np.zeros((10000, 2), np.int16), 44100).ticks()


def test_audio_dropin_stream(native, tmp_path):
    """audio.Audio(filename).audio_stream(): the reference's ints -15 .. 16 for a .wav"""
    import audio
    p = _signal("sine", 150000, 2, 9)
    path = str(tmp_path / "a.wav")
    _write_wav(path, p, 44100)
    a = audio.Audio(path)
    want_norm = M.normalization(p.reshape(-1), 2, 44100)
    assert abs(a.normalization - want_norm) <= 1e-5 * want_norm and a.sample_rate == 14700.0
    got = np.array(list(a.audio_stream()))
    want, v = M.ticks(p.reshape(-1), 2, 44100, a.normalization)
    _check_ticks((2 * got + 34).astype(np.uint8), want, v)


def _write_wav(path, pcm, rate):
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes())


def _tick_offset(k):
    if k < 291:
        return 7 + 7 * k
    g, r = divmod(k - 291, 292)
    return 2048 * (1 + g) + 7 * r


def _opcodes(data, n):
    """(n, 7) bytes of tick opcodes 0 .. n-1 of an .a2m stream"""
    return np.stack([np.frombuffer(data[_tick_offset(k):_tick_offset(k) + 7], np.uint8) for k in range(n)])


@pytest.mark.parametrize("seconds,channels", [(0.4, 2), (1.5, 1)])
def test_transcode_clip_with_audio(native, tmp_path, seconds, channels):
    import stream_batch
    n_frames = int(44100 * seconds)
    pcm = _signal("chirp", n_frames, channels, 11)
    wav = str(tmp_path / "a.wav")
    _write_wav(wav, pcm, 44100)
    tool = os.path.join(ROOT, "tools", "transcode_clip.py")
    out_a, out_t = str(tmp_path / "a.a2m"), str(tmp_path / "t.a2m")
    subprocess.run([sys.executable, tool, "--synthetic", "30", "--audio", wav, "--out", out_a], check=True, timeout=600)
    subprocess.run([sys.executable, tool, "--synthetic", "30", "--tick", "34", "--out", out_t], check=True, timeout=600)
    da, dt = open(out_a, "rb").read(), open(out_t, "rb").read()
    norm = M.normalization(pcm.reshape(-1), channels, 44100)
    want, v = M.ticks(pcm.reshape(-1), channels, 44100, norm)
    clock = stream_batch.MovieClock(True, 14700.0, 30.0)
    n_ops = sum(s[3] for s in clock.segments(30, max_ticks=len(want)))
    assert n_ops == min(len(want), 14699)
    clock_t = stream_batch.MovieClock(True, 14700.0, 30.0)
    n_ops_t = sum(s[3] for s in clock_t.segments(30))
    # the stream's length: its opcodes, the ACKs between, Terminate, and padding to 2 KiB
    end = _tick_offset(n_ops) + 2
    assert len(da) == end + (2048 - end % 2048)
    oa, ot = _opcodes(da, n_ops), _opcodes(dt, n_ops_t)
    # the placeholder addresses the tool uses without --dbg: 0x8000 + 16 * ((tick - 4) / 2 * 32 + page - 32)
    idx = ((oa[:, 0].astype(int) << 8 | oa[:, 1]) - 0x8000) // 16
    ticks, page = 4 + 2 * (idx // 32), 32 + idx % 32
    idx_t = ((ot[:, 0].astype(int) << 8 | ot[:, 1]) - 0x8000) // 16
    assert (4 + 2 * (idx_t // 32) == 34).all()
    _check_ticks(ticks.astype(np.uint8), want[:n_ops], v[:n_ops])
    assert np.array_equal(page, 32 + idx_t[:n_ops] % 32)
    assert np.array_equal(oa[:, 2:], ot[:n_ops, 2:])
