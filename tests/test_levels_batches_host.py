"""CPU: what tests/test_gpu_levels_batches.py and the grid of tests/test_gpu_levels.py rely on without being able to see it.

  the constants   kClipThreads, kClipLanePixels and kClipGridCap are read from the text of csrc/iiv_clip.h, kLevelsApplyFrames
                  from csrc/iiv_levels.hip, and must equal what tests/levels_cases.py mirrors: a changed cap or frame range fails
                  here, instead of passing unnoticed while the GPU tests silently stop reaching the loops' later trips
  the arithmetic  2049 clips of one frame of 8 pixels are the least with a second trip of either kernel, 4097 with a third
  the pool        on the model alone: the seven clips' expected histograms and bytes are pairwise different, so "another clip's
                  result" can never equal the right one"""
import os
import re

import levels_cases as LC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ii-vision_amd", "csrc")


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_levels_constants_equal_the_source():
    with open(os.path.join(CSRC, "iiv_levels.hip")) as f:
        src = f.read()
    with open(os.path.join(CSRC, "iiv_clip.h")) as f:
        clip = f.read()
    assert int(_one(r"constexpr int kClipThreads = (\d+);", clip)) == LC.THREADS
    assert int(_one(r"constexpr int kClipLanePixels = (\d+);", clip)) == LC.LANE_PIXELS
    assert int(_one(r"constexpr int kLevelsApplyFrames = (\d+);", src)) == LC.APPLY_FRAMES
    assert int(_one(r"constexpr int kClipGridCap = (\d+);", clip)) == LC.GRID_CAP
    # the histogram's items are the frames; apply's are clips times runs of lanes times ranges of frames; both grids are capped
    # and both loops stride by the grid
    assert "size_t clip_lanes(long pixels) { return (size_t)pixels / kClipLanePixels; }" in clip
    assert "size_t clip_runs(size_t lanes) { return (lanes + kClipThreads - 1) / kClipThreads; }" in clip
    assert "(unsigned)(n_items < (size_t)kClipGridCap ? n_items : (size_t)kClipGridCap)" in clip
    assert "const size_t n_items = (size_t)n_clips * (size_t)n_frames;" in src
    assert "const size_t lanes = clip_lanes(pixels), runs = clip_runs(lanes);" in src
    assert "const size_t ranges = ((size_t)n_frames + kLevelsApplyFrames - 1) / kLevelsApplyFrames;" in src
    assert "const size_t n_items = (size_t)n_clips * runs * ranges;" in src
    assert " ".join(src.split()).count("dim3(clip_grid(n_items)), dim3(kClipThreads)") == 2
    assert src.count("for (size_t item = blockIdx.x; item < n_items; item += gridDim.x)") == 2
    # the grid's pixel counts sit around a wave and a workgroup, the frame counts of the apply test around a range of frames
    assert {64 * LC.LANE_PIXELS - 4, 64 * LC.LANE_PIXELS, 64 * LC.LANE_PIXELS + 4, LC.THREADS * LC.LANE_PIXELS + 4} <= set(LC.PIXELS)
    assert LC.RANGE_FRAMES == 2 * LC.APPLY_FRAMES + 1


def test_batch_sizes_reach_the_trips():
    assert (LC.N_SECOND, LC.N_THIRD) == (2049, 4097)
    for n in (LC.N_SECOND, LC.N_THIRD):
        LC.assert_trips(n)
    assert LC.apply_items(1, 17, 53760) == 53 * 3 and LC.apply_items(3, 8, 1028) == 6 and LC.hist_items(3, 3) == 9


def test_pool_clips_differ():
    hist, out, lut, m = LC.pool_want()
    assert hist.shape == (7, LC.BATCH_FRAMES, 4, 256) and out.shape == (7, LC.BATCH_FRAMES, LC.BATCH_PIXELS, 3)
    for i in range(7):
        for j in range(i):
            assert (hist[i] != hist[j]).any() and (out[i] != out[j]).any() and (lut[i] != lut[j]).any() and (m[i] != m[j]).any(), (i, j)
    assert (hist.astype(int).sum(axis=-1) == LC.BATCH_PIXELS).all()
