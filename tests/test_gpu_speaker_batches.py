"""GPU: speaker_kernel (csrc/iiv_speaker.hip) past the first trip of its grid-stride loop, as tests/test_gpu_render_batches.py does
for the render kernels.

The kernel walks a list of (stream, run) items, a run being RUN = 2048 consecutive samples, with a grid of at most GRID_CAP = 2048
workgroups.  At decim 73 a sample is a period, so rows of 2040 opcodes (2052 periods) are two runs each and 1025 rows are the
least with a second trip, 2049 with a third.  On a later trip a workgroup restages its LDS widths behind a barrier and keeps the
filter table it copied once in front of the loop.

Row i of every batch is item i % 7 of a pool of seven (tests/speaker_cases.py) with seven different counts -- a full second run, none,
one sample of one, a short stream, an empty one --, gathered on the device; the model runs on the seven and EVERY sample of the
batch is compared, the sentinel behind each row's own count included.  The item a workgroup meets on a later trip lies 1024 or
2048 rows further on: 2 or 4 items further round the pool, never 0.  tests/test_speaker_batches_host.py holds the mirrored
constants to the kernel's text and the seven expected rows pairwise different."""
import numpy as np
import pytest

import speaker_cases as SC
import speaker_model as M

pytestmark = pytest.mark.gpu


def _gather(a, n):
    import torch
    dev = torch.from_numpy(np.array(a)).cuda()
    return dev.index_select(0, torch.arange(n, device="cuda") % SC.P)


@pytest.mark.parametrize("order,gain", [(1, 73), (3, 16384), (4, 32767)])
@pytest.mark.parametrize("n", [SC.N_SECOND, SC.N_THIRD])
def test_every_sample_past_the_first_trip(native, n, order, gain):
    import torch
    SC.assert_trips(n)
    ticks = _gather(SC.pool(), n)
    counts = _gather(np.array(SC.POOL_COUNTS, np.int64), n)
    width = M.sample_count(SC.BATCH_STRIDE, SC.BATCH_DECIM)
    stride = width + 4                                           # 2056: every row starts 16-byte aligned
    out = torch.full((n, stride), SC.SENTINEL, dtype=torch.int16, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    got, m = native.speaker_pcm(ticks, counts, SC.BATCH_DECIM, order, gain, out=out, d_err=err)
    assert got.data_ptr() == out.data_ptr() and int(err.item()) == 0
    assert list(m[:SC.P]) == [M.sample_count(c, SC.BATCH_DECIM) for c in SC.POOL_COUNTS]
    want = torch.from_numpy(np.array(SC.pool_want(order, gain))).cuda()
    bad = torch.zeros(n, dtype=torch.bool, device="cuda")
    for r in range(SC.P):
        bad[r::SC.P] = (out[r::SC.P, :width] != want[r]).any(1)
    idx = torch.nonzero(bad).flatten().cpu().numpy()
    assert len(idx) == 0, "%d of %d rows differ from the model, the first at %s" % (len(idx), n, idx[:10])
    assert bool((out[:, width:] == SC.SENTINEL).all())
