"""GPU: temporal_kernel (csrc/iiv_temporal.hip) past the first trip of its grid-stride loop, as tests/test_gpu_speaker_batches.py does
for the speaker kernel.

The kernel walks a list of (clip, run of 256 lanes) items with a grid of at most GRID_CAP = 2048 workgroups.  Clips of 8 pixels are
one item each, so 2049 clips are the least with a second trip and 4097 with a third; on a later trip a workgroup keeps the weight
table it staged once in front of the loop and takes a new held value, a new ring and a new state row.

Clip i of every batch is item i % 7 of a pool of seven (tests/temporal_cases.py), gathered on the device; the model runs on the seven
and EVERY byte, state and count of the batch is compared.  The clip a workgroup meets on a later trip lies 2048 or 4096 clips further
on: 4 or 1 items further round the pool, never 0.  tests/test_temporal_batches_host.py holds the mirrored constants to the kernel's
text and the seven expected clips pairwise different."""
import numpy as np
import pytest

import temporal_cases as TC

pytestmark = pytest.mark.gpu


def _gather(a, n):
    import torch
    dev = torch.from_numpy(np.array(a)).cuda()
    return dev.index_select(0, torch.arange(n, device="cuda") % TC.P)


@pytest.mark.parametrize("continued", [False, True])
@pytest.mark.parametrize("n", [TC.N_SECOND, TC.N_THIRD])
def test_every_clip_past_the_first_trip(native, n, continued):
    """continued: frame 0 in one call, the rest in a second one from the state: the state rows are read on the later trips too"""
    import torch
    TC.assert_trips(n)
    frames = _gather(TC.pool(), n).view(n, TC.BATCH_FRAMES, 2, 4, 3)
    want, want_state, want_counts = (_gather(a.view(np.int32) if a.dtype == np.uint32 else a, n) for a in TC.pool_want())
    lo, hi = TC.BATCH_PAIR
    if continued:
        a, state, ca = native.temporal_hold(frames[:, :1], lo, hi, counts=True)
        b, state, cb = native.temporal_hold(frames[:, 1:], lo, hi, state=state, counts=True)
        out, counts = torch.cat([a, b], dim=1), torch.cat([ca, cb], dim=1)
    else:
        out, state, counts = native.temporal_hold(frames, lo, hi, counts=True)
    bad = (out.view(n, -1) != want.view(n, -1)).any(1) | (state.view(n, -1) != want_state.view(n, -1)).any(1) \
        | (counts.view(n, -1) != want_counts.view(n, -1)).any(1)
    idx = torch.nonzero(bad).flatten().cpu().numpy()
    assert len(idx) == 0, "%d of %d clips differ from the model, the first at %s" % (len(idx), n, idx[:10])
