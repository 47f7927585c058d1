"""GPU: filter_kernel (csrc/iiv_filter.hip) past the first trip of its grid-stride loop, as tests/test_gpu_temporal_batches.py does for
the temporal hold.

The kernel walks a list of (clip, frame, tile) items with a grid of at most GRID_CAP = 2048 workgroups.  Clips of one 4 x 1 frame are
one item each, so 2049 clips are the least with a second trip and 4097 with a third; with T_h + 1 rows a frame is two tiles, 1025 and
2049 clips are the least, and the two tiles of one frame are taken by different workgroups on different trips.  On a later trip a
workgroup keeps the gain table it staged once in front of the loop and overwrites the rows of h it left in LDS.

Clip i of every batch is item i % 7 of a pool of seven (tests/spatial_cases.py), gathered on the device; the model runs on the seven
and EVERY byte of the batch is compared.  tests/test_spatial_batches_host.py holds the mirrored constants to the kernel's text, the
counts to the trips and the seven expected clips pairwise different."""
import numpy as np
import pytest

import spatial_cases as SC

pytestmark = pytest.mark.gpu


def _gather(a, n):
    import torch
    dev = torch.from_numpy(np.array(a)).cuda()
    return dev.index_select(0, torch.arange(n, device="cuda") % SC.P)


@pytest.mark.parametrize("trip", [2, 3])
@pytest.mark.parametrize("H", SC.BATCH_HEIGHTS)
def test_every_clip_past_the_first_trip(native, H, trip):
    import torch
    n = SC.least_clips(trip, H)
    SC.assert_trips(n, H)
    frames = _gather(SC.pool(H), n)
    want = _gather(SC.pool_want(H), n)
    out = native.filter_frames(frames, SC.BATCH_TAPS[0], SC.BATCH_TAPS[1], SC.GAINS[SC.BATCH_GAIN])
    bad = (out.view(n, -1) != want.view(n, -1)).any(1)
    idx = torch.nonzero(bad).flatten().cpu().numpy()
    assert len(idx) == 0, "%d of %d clips differ from the model, the first at %s" % (len(idx), n, idx[:10])
