"""GPU: levels_histogram_kernel and levels_apply_kernel (csrc/iiv_levels.hip) past the first trip of their grid-stride loops, as
tests/test_gpu_temporal_batches.py does for the temporal hold.

Both kernels walk a list of work items with a grid of at most GRID_CAP = 2048 workgroups: the histogram one item a frame, apply one a
(clip, run of 256 lanes, range of 8 frames).  Clips of one frame of 8 pixels are one item each for both, so 2049 clips are the least
with a second trip and 4097 with a third; on a later trip the histogram's workgroup counts into the bins it cleared while storing
the item before, and apply's stages the tables of a clip it has not met.

Clip i of every batch is item i % 7 of a pool of seven (tests/levels_cases.py) with tables of its own, gathered on the device; the
model runs on the seven and EVERY count and byte of the batch is compared.  The clip a workgroup meets on a later trip lies 2048 or
4096 clips further on: 4 or 1 items further round the pool, never 0.  tests/test_levels_batches_host.py holds the mirrored constants
to the kernels' text and the seven expected clips pairwise different."""
import numpy as np
import pytest

import levels_cases as LC

pytestmark = pytest.mark.gpu


def _gather(a, n):
    import torch
    dev = torch.from_numpy(np.array(a)).cuda()
    return dev.index_select(0, torch.arange(n, device="cuda") % LC.P)


@pytest.mark.parametrize("n", [LC.N_SECOND, LC.N_THIRD])
def test_every_clip_past_the_first_trip(native, n):
    import torch
    LC.assert_trips(n)
    want_hist, want_out, lut, m = LC.pool_want()
    frames = _gather(LC.pool(), n).view(n, LC.BATCH_FRAMES, 2, 4, 3)
    hist = native.levels_histogram(frames)
    bad = (hist.view(n, -1) != _gather(want_hist.view(np.int32), n).view(n, -1)).any(1)
    idx = torch.nonzero(bad).flatten().cpu().numpy()
    assert len(idx) == 0, "%d of %d clips' histograms differ from the model, the first at %s" % (len(idx), n, idx[:10])
    pick = np.arange(n) % LC.P
    out = native.levels_apply(frames, lut[pick], m[pick])
    bad = (out.view(n, -1) != _gather(want_out, n).view(n, -1)).any(1)
    idx = torch.nonzero(bad).flatten().cpu().numpy()
    assert len(idx) == 0, "%d of %d clips differ from the model, the first at %s" % (len(idx), n, idx[:10])
