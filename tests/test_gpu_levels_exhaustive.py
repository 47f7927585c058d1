"""GPU: picture levels over every RGB triple, as tests/test_gpu_yuv_exhaustive.py does for the YUV front door.  All 2^24 triples are
one frame; iiv_levels_apply runs on it for three (table, matrix) pairs -- the identity, a gamma-2.2 table with saturation 512, and
random ones -- and must equal the model (tests/levels_model.py) on every byte; the histogram of the same frame must have every R,
G and B bin at 65 536 and the Y bins of the model.  The comparison runs on the device against the model's bytes; the model itself is
numpy on the host, once per pair."""
import numpy as np
import pytest

import levels_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def triples():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v & 255), (v >> 8) & 255, v >> 16], axis=-1).astype(np.uint8)     # (2^24, 3)


def _pairs():
    import frame_grabber
    rng = np.random.default_rng(1561)
    return {"identity": (M.IDENTITY_LUT, M.IDENTITY_MATRIX),
            "gamma 2.2, saturation 512": (frame_grabber.levels_lut(gamma=2.2), frame_grabber.saturation_matrix(512).astype(np.int64)),
            "random": (rng.integers(0, 256, (3, 256)).astype(np.uint8), rng.integers(-2048, 2048, (3, 3)))}


@pytest.mark.parametrize("name", ["identity", "gamma 2.2, saturation 512", "random"])
def test_apply_on_every_triple(native, triples, name):
    import torch
    lut, m = _pairs()[name]
    frames = torch.from_numpy(triples).cuda().view(1, 4096, 4096, 3)
    got = native.levels_apply(frames, lut, m)
    want = torch.from_numpy(M.apply(triples, lut, m)).cuda().view(1, 4096, 4096, 3)
    bad = int((got != want).any(dim=-1).sum())
    assert bad == 0, "%s: %d of 2^24 triples differ from the model" % (name, bad)
    if name == "identity":
        assert torch.equal(got, frames)


def test_histogram_of_every_triple(native, triples):
    import torch
    hist = native.levels_histogram(torch.from_numpy(triples).cuda().view(1, 4096, 4096, 3)).cpu().numpy().view(np.uint32)[0]
    assert (hist[:3] == 65536).all()
    want_y = np.bincount(M.luma(triples), minlength=256)
    assert np.array_equal(hist[3], want_y) and int(hist[3].astype(np.int64).sum()) == 1 << 24
