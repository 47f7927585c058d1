"""The tests' model of the reference's audio track (transcoder/audio.py, movie.py:104-107), written from the reference's
description with numpy.fft in float64 -- neither librosa nor audioread is needed, and scipy is not assumed.

    decode block   audio.py:98     f.read_data(128 * 1024): blocks of 131072 frames, the last one short
    _decode        audio.py:47-60  int16 -> float32, channel mean (librosa.to_mono), librosa.resample(res_type='scipy',
                                   scale=True): scipy.signal.resample to ceil(n * ratio) samples, / sqrt(ratio)
    _normalization audio.py:60-78  1024-frame reads until more than 10 MiB are held, one block, 16384 / max|percentile|
    audio_stream   audio.py:93-107 a / 16384 * normalization, clip(int(a * 16), -15, 16)
    tick           movie.py:104-107 2 au + 34
"""
import math

import numpy as np

BITRATE = 14700
BLOCK_FRAMES = 128 * 1024
RAW_BLOCK_FRAMES = 1024
PREFIX_BYTES = 1024 * 1024 * 10


def n_out(n_in, rate, bitrate=BITRATE):
    """librosa 0.9.2 resample: ratio = float(target) / orig, int(ceil(n * ratio)), float64; rate == bitrate: n."""
    if rate == bitrate:
        return int(n_in)
    ratio = float(bitrate) / rate
    return int(np.ceil(n_in * ratio))


def blocks(n_frames, block_frames=BLOCK_FRAMES):
    """(first frame, frame count) of every decode block"""
    return [(f, min(block_frames, n_frames - f)) for f in range(0, n_frames, block_frames)]


def tick_count(n_frames, rate, bitrate=BITRATE, block_frames=BLOCK_FRAMES):
    if rate == bitrate:
        return int(n_frames)
    return sum(n_out(n, rate, bitrate) for _, n in blocks(n_frames, block_frames))


def prefix_frames(n_frames, channels):
    """audio.py:62-66: raw blocks of 1024 frames (2 bytes a sample) until len(raw) > 10 MiB, or the end"""
    bpb = RAW_BLOCK_FRAMES * 2 * channels
    return min(n_frames, (PREFIX_BYTES // bpb + 1) * RAW_BLOCK_FRAMES)


def scipy_resample(x, num):
    """scipy.signal.resample(x, num) for real 1-D x, in float64 (scipy/signal/_signaltools.py: rfft, keep
    min(num, Nx) // 2 + 1 bins, the even Nyquist bin x2 when downsampling and x0.5 when upsampling, irfft(num),
    * num / Nx)."""
    x = np.asarray(x, dtype=np.float64)
    nx = len(x)
    X = np.fft.rfft(x)
    Y = np.zeros(num // 2 + 1, dtype=np.complex128)
    N = min(num, nx)
    nyq = N // 2 + 1
    Y[:nyq] = X[:nyq]
    if N % 2 == 0:
        if num < nx:
            Y[N // 2] *= 2.0
        elif nx < num:
            Y[N // 2] *= 0.5
    return np.fft.irfft(Y, num) * (float(num) / float(nx))


def mono(pcm, channels):
    """interleaved int16 (n * channels,) -> float64 channel mean (exact for int16 inputs up to rounding of the mean)"""
    a = np.asarray(pcm, dtype=np.int16).reshape(-1, channels).astype(np.float64)
    return a.mean(axis=1)


def decode(pcm, channels, rate, bitrate=BITRATE):
    """audio.Audio._decode of one block (audio.py:47-60)"""
    y = mono(pcm, channels)
    if rate == bitrate:
        return y
    ratio = float(bitrate) / rate
    return scipy_resample(y, n_out(len(y), rate, bitrate)) / math.sqrt(ratio)


def stream_values(pcm, channels, rate, bitrate=BITRATE, block_frames=BLOCK_FRAMES):
    """every decoded block of a stream, concatenated (float64)"""
    pcm = np.asarray(pcm, dtype=np.int16).reshape(-1, channels)
    n = len(pcm)
    if rate == bitrate:
        return decode(pcm.reshape(-1), channels, rate, bitrate)
    return np.concatenate([decode(pcm[f:f + k].reshape(-1), channels, rate, bitrate) for f, k in blocks(n, block_frames)]
                          or [np.zeros(0)])


def normalization(pcm, channels, rate, bitrate=BITRATE):
    """audio.Audio._normalization (audio.py:60-78)"""
    pcm = np.asarray(pcm, dtype=np.int16).reshape(-1, channels)
    p = prefix_frames(len(pcm), channels)
    a = decode(pcm[:p].reshape(-1), channels, rate, bitrate)
    norm = np.max(np.abs(np.percentile(a, [0.5, 99.5])))
    return 16384. / norm


def ticks_from_values(a, norm):
    """audio.py:100-105 + movie.py:104-107 -> (uint8 ticks, float64 a * 16 before truncation)"""
    v = np.asarray(a, dtype=np.float64) / 16384 * norm * 16
    au = np.clip(np.trunc(v), -15, 16).astype(np.int64)
    return (2 * au + 34).astype(np.uint8), v


def ticks(pcm, channels, rate, norm, bitrate=BITRATE, block_frames=BLOCK_FRAMES):
    return ticks_from_values(stream_values(pcm, channels, rate, bitrate, block_frames), norm)


# ---- what the GPU tests and tests/stage_fuzz.py share: the test signals and the criterion for ticks --------------------

SIGNAL_KINDS = ("sine", "chirp", "noise", "loud")


def signal(kind, n, channels, seed):
    """int16 (n, channels)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    if kind == "sine":
        x = 9000 * np.sin(2 * np.pi * 440 * t) + 4000 * np.sin(2 * np.pi * 3111 * t + 1)
    elif kind == "chirp":
        x = 12000 * np.sin(2 * np.pi * (50 * t + 4000 * t * t))
    elif kind == "noise":
        x = rng.normal(0, 6000, n)
    elif kind == "loud":   # clipping-heavy: mostly beyond the 0.5 / 99.5 percentiles' range after normalisation
        x = 32000 * np.sign(np.sin(2 * np.pi * 97 * t)) + rng.normal(0, 3000, n)
    else:
        raise ValueError(kind)
    out = np.empty((n, channels))
    for c in range(channels):
        out[:, c] = x * (1.0 - 0.3 * c) + rng.normal(0, 200, n)
    return np.clip(np.round(out), -32768, 32767).astype(np.int16)


def check_ticks(got, want, v):
    """equal, except within 1e-3 of an integer of the model's a * 16 (one level), fewer than 0.5 % of the samples"""
    bad = got != want
    near = np.abs(v - np.round(v)) < 1e-3
    assert not (bad & ~near).any(), "ticks differ away from a level boundary at %s" % np.nonzero(bad & ~near)[0][:10]
    assert (np.abs(got.astype(int) - want.astype(int))[bad] <= 2).all()
    assert bad.sum() < 0.005 * max(len(want), 1)
