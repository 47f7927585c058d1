"""CPU: the audio track's host side -- the tests' model of the reference (tests/audio_model.py) against scipy, the tick
count arithmetic of the C ABI, decode blocks and the normalisation prefix, the .wav reader, and no CPU fallback."""
import os
import wave

import numpy as np
import pytest

import audio_model as M


@pytest.mark.parametrize("nx,num", [(8, 3), (9, 3), (8, 4), (9, 4), (7, 12), (8, 12), (8, 13), (1, 1), (2, 1), (3, 1),
                                    (2048, 683), (2047, 683), (683, 1255), (4097, 1366), (10, 10)])
def test_model_resample_equals_scipy(nx, num):
    """scipy.signal.resample of real input: even / odd N and num, down- and upsampling (skipped without scipy)"""
    signal = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(nx * 1000 + num).standard_normal(nx)
    want = signal.resample(x, num)
    got = M.scipy_resample(x, num)
    assert got.shape == (num,)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()))


def test_model_decode_scale_and_identity():
    """librosa.resample(scale=True) divides by sqrt(target / orig); orig == target returns the mono signal as is"""
    signal = pytest.importorskip("scipy.signal")
    pcm = np.random.default_rng(1).integers(-20000, 20000, size=(3000, 2)).astype(np.int16)
    y = pcm.astype(np.float64).mean(axis=1)
    for rate in (44100, 48000, 8000, 22050):
        num = int(np.ceil(3000 * (14700.0 / rate)))
        want = signal.resample(y, num) / np.sqrt(14700.0 / rate)
        np.testing.assert_allclose(M.decode(pcm.reshape(-1), 2, rate), want, atol=1e-9 * np.abs(want).max())
    assert np.array_equal(M.decode(pcm.reshape(-1), 2, 14700), y)


def test_n_out_float64_arithmetic(native):
    """int(ceil(n * (target / orig))) in float64: exact multiples stay exact (3 frames at 44100 -> 1 tick)"""
    assert M.n_out(3, 44100) == 1
    assert M.n_out(131072, 44100) == 43691
    assert M.n_out(2048, 44100) == 683
    assert M.n_out(2622464, 44100) == 874155
    rng = np.random.default_rng(2)
    for rate in (8000, 11025, 22050, 32000, 44100, 48000, 96000, 14700, 29400):
        for n in list(range(1, 200)) + [131072, 2048, 2622464] + list(rng.integers(1, 3_000_000, 50)):
            want = int(n) if rate == 14700 else int(np.ceil(int(n) * (14700.0 / rate)))
            assert M.n_out(int(n), rate) == want
            assert native.audio_tick_count(int(n), rate, 14700, 1 << 30) == want, (n, rate)


def test_tick_count_over_blocks(native):
    """the stream is decoded in blocks of 131072 frames (audio.py:98), the last one short; each is resampled alone"""
    assert M.blocks(300000, 131072) == [(0, 131072), (131072, 131072), (262144, 37856)]
    for n, rate, bf in [(300000, 44100, 131072), (1455300, 44100, 131072), (1455300, 48000, 2048), (99999, 22050, 3001),
                        (5, 44100, 2), (0, 44100, 131072), (131072, 44100, 131072), (1000, 14700, 7)]:
        want = sum(M.n_out(k, rate) for _, k in M.blocks(n, bf)) if rate != 14700 else n
        assert M.tick_count(n, rate, block_frames=bf) == want
        assert native.audio_tick_count(n, rate, 14700, bf) == want
    with pytest.raises(RuntimeError):
        native.audio_tick_count(10, 0, 14700, 131072)


def test_normalisation_prefix_length():
    """1024-frame reads until more than 10 MiB are held: stereo 2561 reads = 2 622 464 frames, mono 5121 reads"""
    assert M.prefix_frames(10 ** 8, 2) == 2622464
    assert M.prefix_frames(10 ** 8, 1) == 5121 * 1024
    assert M.prefix_frames(10 ** 8, 6) == (10485760 // 12288 + 1) * 1024
    assert M.prefix_frames(1000, 2) == 1000


def _write_wav(path, pcm, rate, width=2):
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes() if width == 2 else pcm.astype(np.uint8).tobytes())


def test_wav_reader(tmp_path):
    import audio
    pcm = np.random.default_rng(3).integers(-32768, 32767, size=(5000, 2)).astype(np.int16)
    p = str(tmp_path / "a.wav")
    _write_wav(p, pcm, 44100)
    got, rate = audio.read_wav(p)
    assert rate == 44100 and got.dtype == np.int16 and np.array_equal(got, pcm)
    p8 = str(tmp_path / "b.wav")
    _write_wav(p8, np.zeros((10, 1), np.uint8), 8000, width=1)
    with pytest.raises(ValueError, match="16-bit"):
        audio.read_wav(p8)
    mp3 = str(tmp_path / "c.mp3")
    with open(mp3, "wb") as f:
        f.write(b"ID3\x03\x00" + bytes(100))
    with pytest.raises(ValueError, match="decoder"):
        audio.read_wav(mp3)


def test_audio_entries_raise_without_gpu(native):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    pcm = torch.zeros((1, 10), dtype=torch.int16)
    for call in (lambda: native.audio_ticks(pcm, 10, 1, 44100, 1.0), lambda: native.audio_normalization(pcm, 10, 1, 44100),
                 lambda: native.audio_resample(pcm, 10, 1, 44100)):
        with pytest.raises(RuntimeError):
            call()
    import audio
    with pytest.raises(RuntimeError):
        audio.ArrayAudio(np.zeros((100, 2), np.int16), 44100, normalization=1.0)


def test_audio_module_has_the_reference_interface():
    import inspect
    import audio
    sig = inspect.signature(audio.Audio.__init__)
    assert list(sig.parameters) == ["self", "filename", "bitrate", "normalization"]
    assert sig.parameters["bitrate"].default == 14700 and sig.parameters["normalization"].default is None
    src = open(audio.__file__).read()
    assert "import oracle" not in src and "audio_model" not in src


def test_prefix_rule_of_the_binding_matches_the_model(native):
    for n, ch in [(10 ** 8, 1), (10 ** 8, 2), (10 ** 8, 6), (1000, 2), (2622464, 2), (5243904, 1)]:
        assert native.audio_prefix_frames(n, ch) == M.prefix_frames(n, ch)
