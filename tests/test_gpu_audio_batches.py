"""GPU: csrc/iiv_audio.hip past its first chunk and at its largest transform, against the tests' model
(tests/audio_model.py, float64).  run_group cuts the jobs of one (nx, num) group into chunks that fit a 1 GiB work buffer
(iiv_audio.hip:373 kWorkspaceBytes, :404-411), at most 65535 jobs; the transforms go up to 2^24 points (:215-216).

The batches are periodic: stream s is base[s % P] with P = 7, prime to every chunk size below, so the model runs P times
and a chunk that reads or writes the wrong jobs lands on different content.  The bounds are those of test_gpu_audio.py."""
import numpy as np
import pytest

import audio_model as M
from audio_model import check_ticks as _check_ticks, signal as _signal

pytestmark = pytest.mark.gpu

P = 7
WORKSPACE_BYTES = 1 << 30    # iiv_audio.hip:373 kWorkspaceBytes: one work buffer of a group
MAX_CHUNK_JOBS = 65535       # iiv_audio.hip:405
KINDS = ("noise", "chirp", "sine", "loud")


def transform_points(n):
    """iiv_audio.hip transform_points: n for a power of two, else Bluestein's next power of two >= 2n - 1"""
    if n & (n - 1) == 0:
        return n
    m = 1
    while m < 2 * n - 1:
        m <<= 1
    return m


def chunk_jobs(nx, num):
    """jobs per chunk of the group (nx, num) (iiv_audio.hip:404-405)"""
    lmax = max(transform_points(nx), transform_points(num))
    return max(1, min(WORKSPACE_BYTES // (8 * lmax), MAX_CHUNK_JOBS))


def _bases(n_frames, channels, seed):
    """P int16 (n_frames, channels) signals"""
    return [_signal(KINDS[k % len(KINDS)], n_frames, channels, seed + k) for k in range(P)]


def _periodic_pcm(bases, n_streams):
    """CUDA int16 (n_streams, max samples): row s = base[s % P]"""
    import torch
    width = max(b.size for b in bases)
    host = np.zeros((P, width), np.int16)
    for k, b in enumerate(bases):
        host[k, :b.size] = b.reshape(-1)
    return torch.from_numpy(host).cuda()[torch.arange(n_streams, device="cuda") % P]


def _ticks_across_chunks(native, n_streams, n_frames, channels, block_frames, seed):
    import torch
    bases = _bases(n_frames, channels, seed)
    pcm = _periodic_pcm(bases, n_streams)
    base_norm = [M.normalization(b.reshape(-1), channels, 44100) for b in bases]
    # each stream its own normalisation: a mix-up between streams of the same base shows too
    norms = [base_norm[s % P] * (0.6 + 0.05 * (s % 13)) for s in range(n_streams)]
    count = M.tick_count(n_frames, 44100, block_frames=block_frames)
    out = torch.full((n_streams, count + 64), 0xAB, dtype=torch.uint8, device="cuda")
    t, counts = native.audio_ticks(pcm, n_frames, channels, 44100, norms, block_frames=block_frames, out=out)
    assert t is out and (counts == count).all()
    host = out.cpu().numpy()
    del pcm, out, t
    torch.cuda.empty_cache()
    values = [M.stream_values(b.reshape(-1), channels, 44100, block_frames=block_frames) for b in bases]
    for s in range(n_streams):
        want, v = M.ticks_from_values(values[s % P], norms[s])
        assert len(want) == count
        _check_ticks(host[s, :count], want, v)
        assert (host[s, count:] == 0xAB).all(), "stream %d: bytes past the tick count were written" % s


def test_ticks_131072_frame_blocks_across_chunks(native):
    """1100 mono streams of two 131072-frame blocks: 2200 jobs of the group (131072, 43691), chunks of 1024, 1024, 152"""
    nx = M.BLOCK_FRAMES
    num = M.n_out(nx, 44100)
    assert num == 43691 and chunk_jobs(nx, num) == 1024
    _ticks_across_chunks(native, 1100, 2 * nx, 1, nx, 11)


def test_ticks_2048_frame_blocks_past_65535_jobs(native):
    """64 stereo streams of 1100 blocks of 2048 frames: 70400 jobs of the group (2048, 683), chunks of 65535 and 4865"""
    nx = 2048
    assert chunk_jobs(nx, M.n_out(nx, 44100)) == MAX_CHUNK_JOBS
    _ticks_across_chunks(native, 64, 1100 * nx, 2, nx, 21)


def test_resample_across_chunks(native):
    """1100 streams (mono and stereo) of 131072 frames, one job each: chunks of 1024 and 76"""
    import torch
    n_streams, nx = 1100, M.BLOCK_FRAMES
    assert chunk_jobs(nx, M.n_out(nx, 44100)) == 1024
    bases = [_signal(KINDS[k % len(KINDS)], nx, 1 + k % 2, 31 + k) for k in range(P)]
    pcm = _periodic_pcm(bases, n_streams)
    ch = [bases[s % P].shape[1] for s in range(n_streams)]
    y, lens = native.audio_resample(pcm, nx, ch, 44100)
    host = y.cpu().numpy()
    del pcm, y
    torch.cuda.empty_cache()
    for k, b in enumerate(bases):
        want = M.decode(b.reshape(-1), b.shape[1], 44100)
        assert (lens[k::P] == len(want)).all()
        err = np.abs(host[k::P, :len(want)] - want).max(axis=1)
        bad = np.nonzero(err > 1e-5 * np.abs(want).max())[0]
        assert len(bad) == 0, "streams %s: max error %g of max |y| %g" % (k + P * bad[:10], err.max(), np.abs(want).max())


@pytest.fixture(scope="module")
def clip_2_24():
    """one mono 44.1 kHz clip of 2^24 frames (380 s) and the model of its decode as one block"""
    n = 1 << 24
    pcm = _signal("noise", n, 1, 41)
    pcm[: n // 2] = np.clip(pcm[: n // 2].astype(np.int32) + _signal("sine", n // 2, 1, 42), -32768, 32767)
    return pcm, M.decode(pcm.reshape(-1), 1, 44100)


def test_resample_2_24_points(native, clip_2_24):
    """the forward transform is the four-step at a = 24 (2^12 x 2^12), the inverse a Bluestein transform of 5592406
    points on 2^24"""
    import torch
    pcm, want = clip_2_24
    n = pcm.shape[0]
    assert len(want) == 5592406 and transform_points(n) == transform_points(len(want)) == 1 << 24
    y, lens = native.audio_resample(torch.from_numpy(pcm.reshape(1, -1)).cuda(), n, 1, 44100)
    assert lens[0] == len(want)
    err = np.abs(y[0].cpu().numpy().astype(np.float64) - want).max()
    print("2^24 resample: max error %.3g of max |y| %.6g (%.3g)" % (err, np.abs(want).max(), err / np.abs(want).max()))
    assert err <= 1e-5 * np.abs(want).max(), "max error %g of max |y| %g" % (err, np.abs(want).max())


def test_normalization_2_24_points(native, clip_2_24):
    """the normalisation prefix of a mono 44.1 kHz clip is 5243904 frames: a Bluestein forward transform on 2^24"""
    import torch
    pcm = clip_2_24[0]
    p = M.prefix_frames(pcm.shape[0], 1)
    assert p == 5243904 and transform_points(p) == 1 << 24
    got = native.audio_normalization(torch.from_numpy(pcm.reshape(1, -1)).cuda(), pcm.shape[0], 1, 44100)[0]
    want = M.normalization(pcm.reshape(-1), 1, 44100)
    print("2^24 normalisation: relative error %.3g" % (abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)


def test_ticks_2_24_frame_block(native, clip_2_24):
    import torch
    pcm, values = clip_2_24
    n = pcm.shape[0]
    norm = M.normalization(pcm.reshape(-1), 1, 44100)
    out = torch.full((1, len(values) + 64), 0xAB, dtype=torch.uint8, device="cuda")
    _, counts = native.audio_ticks(torch.from_numpy(pcm.reshape(1, -1)).cuda(), n, 1, 44100, norm, block_frames=n, out=out)
    assert counts[0] == len(values)
    host = out.cpu().numpy()[0]
    want, v = M.ticks_from_values(values, norm)
    _check_ticks(host[:len(values)], want, v)
    assert (host[len(values):] == 0xAB).all()


def test_normalization_of_many_streams(native):
    """2000 streams of distinct short lengths and loudness: one radix-select histogram per stream, each value checked"""
    import torch
    n_streams = 2000
    lengths = [300 + 3 * s for s in range(n_streams)]
    channels = [1 + s % 2 for s in range(n_streams)]
    rng = np.random.default_rng(51)
    noise = _signal("noise", max(lengths) + n_streams, 2, 52).astype(np.float64)
    host = np.zeros((n_streams, 2 * max(lengths)), np.int16)
    pcms = []
    for s in range(n_streams):
        gain = 0.1 + 0.9 * ((37 * s) % 101) / 100
        p = np.round(noise[s:s + lengths[s], :channels[s]] * gain + rng.normal(0, 50, (lengths[s], channels[s])))
        p = np.clip(p, -32768, 32767).astype(np.int16)
        host[s, :p.size] = p.reshape(-1)
        pcms.append(p)
    got = native.audio_normalization(torch.from_numpy(host).cuda(), lengths, channels, 44100)
    want = np.array([M.normalization(p.reshape(-1), p.shape[1], 44100) for p in pcms])
    bad = np.nonzero(np.abs(got - want) > 1e-5 * np.abs(want))[0]
    assert len(bad) == 0, "streams %s: got %s, want %s" % (bad[:10], got[bad[:10]], want[bad[:10]])
