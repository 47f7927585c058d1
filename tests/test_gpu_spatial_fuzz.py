"""GPU: seeded differential fuzz of the spatial filter (csrc/iiv_filter.hip) against tests/spatial_model.py: random heights and widths
within 1..40 and 4..64, random frame and clip counts, random padded strides on both sides, random valid taps and random gains, on
inputs that mix noise with flat patches.  A failure prints its seed."""
import numpy as np
import pytest

import spatial_model as M
from device_guards import ok
from stream_cases import dp as _dp

pytestmark = pytest.mark.gpu

ROUNDS = 12
SENTINEL = 0x5B


def _taps(rng):
    cuts = np.sort(rng.integers(0, 257, 4))
    return np.diff(np.concatenate([[0], cuts, [256]])).astype(np.uint16)


def _gain(rng):
    kind = int(rng.integers(0, 3))
    if kind == 0:
        return rng.integers(-256, 1025, 256).astype(np.int16)
    if kind == 1:       # small steps: neighbouring m take neighbouring gains
        return np.clip(np.cumsum(rng.integers(-9, 12, 256)) - 256, -256, 1024).astype(np.int16)
    g = np.zeros(256, np.int16)
    g[:int(rng.integers(1, 40))] = -256
    g[int(rng.integers(40, 200)):] = int(rng.integers(0, 1025))
    return g


@pytest.mark.parametrize("seed", [1620 + i for i in range(ROUNDS)])
def test_round(native, seed):
    import torch
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 41)), 4 * int(rng.integers(1, 17))
    c, n = int(rng.integers(1, 4)), int(rng.integers(1, 5))
    fb = H * W * 3
    sfs, ofs = fb + 4 * int(rng.integers(0, 6)), fb + 4 * int(rng.integers(0, 6))
    scs, ocs = sfs * n + 4 * int(rng.integers(0, 6)), ofs * n + 4 * int(rng.integers(0, 6))
    x = rng.integers(0, 256, (c, n, H, W, 3))
    flat = rng.integers(0, 256, (c, n, 1, 1, 3)) + rng.integers(-6, 7, (c, n, H, W, 3))
    x = np.clip(np.where(rng.integers(0, 2, (c, n, H, W, 1)) == 1, x, flat), 0, 255).astype(np.uint8)
    if seed % 3 == 0:
        x = np.clip(flat, 0, 255).astype(np.uint8)          # noise on a flat frame: the small m of a denoise
    tx, ty, g = _taps(rng), _taps(rng), _gain(rng)
    want = M.filter_frames(x, tx, ty, g)
    src = torch.full((c * scs,), 0x33, dtype=torch.uint8, device="cuda")
    torch.as_strided(src, (c, n, fb), (scs, sfs, 1)).copy_(torch.from_numpy(x).cuda().view(c, n, fb))
    out = torch.full((c * ocs,), SENTINEL, dtype=torch.uint8, device="cuda")
    ok(native, native.lib().iiv_filter_frames(c, n, H, W, _dp(src), scs, sfs, _dp(out), ocs, ofs, native.hptr(tx), native.hptr(ty),
                                              native.hptr(g), native.stream_ptr()))
    got = out.cpu().numpy()
    owned = np.zeros(c * ocs, bool)
    label = "seed %d: %d x %d, %d frames, %d clips, strides %s, taps %s %s" % (seed, H, W, n, c, (scs, sfs, ocs, ofs), tx.tolist(), ty.tolist())
    for k in range(c):
        for t in range(n):
            at = k * ocs + t * ofs
            owned[at:at + fb] = True
            bad = np.argwhere(got[at:at + fb].reshape(H, W, 3) != want[k, t])
            assert len(bad) == 0, "%s: clip %d frame %d: %d bytes differ, the first at %s" % (label, k, t, len(bad), bad[:4].tolist())
    assert (got[~owned] == SENTINEL).all(), label + ": the call wrote into the padding"
