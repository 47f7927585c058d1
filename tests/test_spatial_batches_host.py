"""CPU: what tests/test_gpu_spatial_batches.py and the grid of tests/test_gpu_spatial.py rely on without being able to see it.

  the constants   kClipThreads, kClipLanePixels and kClipGridCap are read from the text of csrc/iiv_clip.h, kFilterTileH,
                  kFilterTileW and kFilterHalo from csrc/iiv_filter.hip, and must equal what tests/spatial_cases.py mirrors: a changed
                  tile or cap fails here, instead of passing unnoticed while the GPU tests silently stop meeting the seams or the
                  loop's later trips
  the arithmetic  2049 clips of one 4 x 1 frame are the least with a second trip and 4097 with a third; with T_h + 1 rows -- two tiles
                  a frame -- 1025 and 2049
  the pool        on the model alone: the seven clips' expected outputs are pairwise different, so "another clip's bytes" can never
                  equal the right ones"""
import os
import re

import spatial_cases as SC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ii-vision_amd", "csrc")


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_spatial_constants_equal_the_source():
    with open(os.path.join(CSRC, "iiv_filter.hip")) as f:
        src = f.read()
    with open(os.path.join(CSRC, "iiv_clip.h")) as f:
        clip = f.read()
    assert int(_one(r"constexpr int kClipThreads = (\d+);", clip)) == SC.THREADS
    assert int(_one(r"constexpr int kClipLanePixels = (\d+);", clip)) == SC.LANE_PIXELS
    assert int(_one(r"constexpr int kClipGridCap = (\d+);", clip)) == SC.GRID_CAP
    assert int(_one(r"constexpr int kFilterTileH = (\d+);", src)) == SC.T_H
    assert int(_one(r"constexpr int kFilterTileW = (\d+);", src)) == SC.T_W
    assert int(_one(r"constexpr int kFilterHalo = (\d+);", src)) == SC.HALO
    assert SC.T_W % SC.LANE_PIXELS == 0
    # the list of items is clips times frames times tiles, the grid is capped, and the loop strides by the grid
    flat = " ".join(src.split())
    assert "(unsigned)(n_items < (size_t)kClipGridCap ? n_items : (size_t)kClipGridCap)" in clip
    assert "const int tiles_y = (height + kFilterTileH - 1) / kFilterTileH, tiles_x = (width + kFilterTileW - 1) / kFilterTileW;" in flat
    assert "const size_t n_items = (size_t)n_clips * (size_t)n_frames * (size_t)tiles_y * (size_t)tiles_x;" in flat
    assert "dim3(clip_grid(n_items)), dim3(kClipThreads)" in flat
    assert "for (size_t item = blockIdx.x; item < n_items; item += gridDim.x)" in src
    # the grid's heights and widths sit around the tile
    assert {SC.T_H - 1, SC.T_H, SC.T_H + 1, 2 * SC.T_H + 3, 1, 2, 3, 4, 5, 192} == set(SC.HEIGHTS)
    assert {SC.T_W - 4, SC.T_W, SC.T_W + 4, 4, 8, 12, 280, 560} == set(SC.WIDTHS)
    assert SC.tiles(192, 280) == 12 and SC.tiles(192, 560) == 24 and SC.tiles(SC.T_H, SC.T_W) == 1 and SC.tiles(SC.T_H + 1, SC.T_W + 4) == 4


def test_batch_sizes_reach_the_trips():
    assert [SC.least_clips(t, 1) for t in (2, 3)] == [2049, 4097]
    assert [SC.least_clips(t, SC.T_H + 1) for t in (2, 3)] == [1025, 2049]
    for H in SC.BATCH_HEIGHTS:
        assert SC.tiles(H, SC.BATCH_W) == (1 if H == 1 else 2)
        for trip in (2, 3):
            SC.assert_trips(SC.least_clips(trip, H), H)


def test_pool_clips_differ():
    for H in SC.BATCH_HEIGHTS:
        src, out = SC.pool(H), SC.pool_want(H)
        assert out.shape == (SC.P, SC.BATCH_FRAMES, H, SC.BATCH_W, 3) and (out != src).any()
        for i in range(SC.P):
            for j in range(i):
                assert (out[i] != out[j]).any(), (H, i, j)
                if H > 1:   # tile by tile as well: a workgroup that took the right clip's other tile is seen
                    assert (out[i, :, :SC.T_H] != out[j, :, :SC.T_H]).any() and (out[i, :, SC.T_H:] != out[j, :, SC.T_H:]).any()
