"""GPU: the audio track's device memory is scoped to a call -- batches of streams of many distinct lengths (each length its
own Bluestein tables) leave nothing behind -- and what it refuses, it refuses before launching anything."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _free_after(torch, fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def test_distinct_lengths_leave_no_memory_behind(native):
    import torch
    rng = np.random.default_rng(4)
    n_streams, width = 24, 2 * 520000
    pcm = torch.randint(-20000, 20000, (n_streams, width), dtype=torch.int16, device="cuda")
    out = torch.empty((n_streams, 200000), dtype=torch.uint8, device="cuda")

    def batch():
        nf = rng.choice(np.arange(300000, 520000), n_streams, replace=False)   # distinct whole-stream and last-block lengths
        y, _ = native.audio_resample(pcm, nf, 2, 44100)
        del y
        native.audio_ticks(pcm, nf, 2, 44100, 2.0, out=out)

    base = _free_after(torch, batch)
    after = base
    for _ in range(3):
        after = _free_after(torch, batch)
    assert base - after < 256 << 20, "device memory grew by %d MiB over three batches" % ((base - after) >> 20)


def test_transform_limit_refused_before_launch(native):
    """8 kHz mono resampled as one block past 2^23 output samples needs a 2^25-point Bluestein transform"""
    import torch
    n = 9_000_000
    pcm = torch.zeros((1, n), dtype=torch.int16, device="cuda")
    with pytest.raises(native.IIVError) as e:
        native.audio_resample(pcm, n, 1, 8000)
    assert e.value.code == native.ERR_INVALID and "2^24" in str(e.value)
    pcm[0, ::7] = 1000
    norm = native.audio_normalization(pcm[:, :n], 4_000_000, 1, 8000)   # a prefix within the limit runs
    assert np.isfinite(norm[0]) and norm[0] > 0


def test_narrow_pcm_view_refused(native):
    import torch
    pcm = torch.zeros((2, 1000), dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError):
        native.audio_ticks(pcm[:, :500], 400, 2, 44100, 1.0)
    with pytest.raises(ValueError):
        native.audio_normalization(pcm[:, :500], 300, 2, 44100)

