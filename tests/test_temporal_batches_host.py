"""CPU: what tests/test_gpu_temporal_batches.py and the grid of tests/test_gpu_temporal.py rely on without being able to see it.

  the constants   kClipThreads, kClipLanePixels and kClipGridCap are read from the text of csrc/iiv_clip.h, kTemporalRing from
                  csrc/iiv_temporal.hip, and must equal what tests/temporal_cases.py mirrors: a changed cap or ring depth fails here,
                  instead of passing unnoticed while the GPU tests silently stop reaching the loop's later trips or the ring's turn
  the arithmetic  2049 clips of 8 pixels are the least with a second trip, 4097 with a third
  the pool        on the model alone: the seven clips' expected outputs are pairwise different, so "another clip's bytes" can never
                  equal the right ones"""
import os
import re

import temporal_cases as TC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ii-vision_amd", "csrc")


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_temporal_constants_equal_the_source():
    with open(os.path.join(CSRC, "iiv_temporal.hip")) as f:
        src = f.read()
    with open(os.path.join(CSRC, "iiv_clip.h")) as f:
        clip = f.read()
    assert int(_one(r"constexpr int kClipThreads = (\d+);", clip)) == TC.THREADS
    assert int(_one(r"constexpr int kClipLanePixels = (\d+);", clip)) == TC.LANE_PIXELS
    assert int(_one(r"constexpr int kTemporalRing = (\d+);", src)) == TC.RING
    assert int(_one(r"constexpr int kClipGridCap = (\d+);", clip)) == TC.GRID_CAP
    # the list of items is clips times runs of lanes, the grid is capped, and the loop strides by the grid
    assert "size_t clip_lanes(long pixels) { return (size_t)pixels / kClipLanePixels; }" in clip
    assert "size_t clip_runs(size_t lanes) { return (lanes + kClipThreads - 1) / kClipThreads; }" in clip
    assert "(unsigned)(n_items < (size_t)kClipGridCap ? n_items : (size_t)kClipGridCap)" in clip
    assert "const size_t lanes = clip_lanes(pixels), runs = clip_runs(lanes);" in src
    assert "const size_t n_items = (size_t)n_clips * runs;" in src
    assert "dim3(clip_grid(n_items)), dim3(kClipThreads)" in " ".join(src.split())
    assert "for (size_t item = blockIdx.x; item < n_items; item += gridDim.x)" in src
    # the grid's frame counts sit around the ring's depth, its pixel counts around a wave and a workgroup
    assert set(TC.N_FRAMES) == {1, 2, 3, TC.RING, TC.RING + 1, 2 * TC.RING + 1}
    assert {64 * TC.LANE_PIXELS - 4, 64 * TC.LANE_PIXELS, 64 * TC.LANE_PIXELS + 4, TC.THREADS * TC.LANE_PIXELS + 4} <= set(TC.PIXELS)


def test_batch_sizes_reach_the_trips():
    assert (TC.N_SECOND, TC.N_THIRD) == (2049, 4097)
    for n in (TC.N_SECOND, TC.N_THIRD):
        TC.assert_trips(n)
    assert TC.runs_per_clip(53760) == 53 and TC.runs_per_clip(1028) == 2 and TC.runs_per_clip(1024) == 1


def test_pool_clips_differ():
    out, state, counts = TC.pool_want()
    assert out.shape == (7, TC.BATCH_FRAMES, TC.BATCH_PIXELS, 3)
    for i in range(7):
        for j in range(i):
            assert (out[i, 0] != out[j, 0]).any() and (state[i] != state[j]).any(), (i, j)
    # the pool holds, blends and passes pixels behind frame 0
    assert counts[:, 1:].sum(axis=(0, 1)).min() > 0 and (counts.astype(int).sum(axis=2) == TC.BATCH_PIXELS).all()
