"""CPU: what tests/test_gpu_render_batches.py and tests/test_gpu_mono_batches.py rely on without being able to see it.

  the constants   kRenderWaves, kRenderRunsPerFrame and the cap in render_grid are read from the text of csrc/iiv_render.h, the
                  default chunk from csrc/iiv_mono.hip, and must equal what the two GPU files mirror: a changed cap fails here,
                  instead of passing unnoticed while the GPU tests silently stop reaching the loops
  the arithmetic  79 frames are the least with a second trip, 157 with a third; 2051 frames are a chunk of 2048 and one of 3
  the pools       on the models alone: the seven items' expected outputs -- the RGB in every palette, each of the nine sums at
                  both reference widths, the mono maps of both banks -- are pairwise different, so "the wrong frame" can never
                  equal the right one"""
import os
import re

import numpy as np
import pytest

import mono_model as M
import test_gpu_mono_batches as MB
import test_gpu_render_batches as RB

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ii-vision_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_render_constants_equal_the_header():
    h = _text("iiv_render.h")
    assert int(_one(r"constexpr int kRenderWaves = (\d+);", h)) == RB.RENDER_WAVES
    assert int(_one(r"constexpr int kRenderRunsPerFrame = (\d+);", h)) == RB.RUNS_PER_FRAME
    grid = h[h.index("static inline unsigned render_grid(size_t n_runs)"):]
    grid = grid[:grid.index("\n}\n")]
    assert "(n_runs + kRenderWaves - 1) / kRenderWaves" in grid
    below, cap = _one(r"return \(unsigned\)\(blocks < (\d+) \? blocks : (\d+)\);", grid)
    assert int(below) == int(cap) == RB.GRID_CAP
    assert RB.RUNS_PER_TRIP == RB.GRID_CAP * RB.RENDER_WAVES == 8192
    # both kernels stride by the whole grid's waves, and both launches take their grid from render_grid
    for name in ("iiv_render.hip", "iiv_render_error.hip"):
        src = _text(name)
        assert "const size_t n_waves = (size_t)gridDim.x * kRenderWaves;" in src, name
        assert "run < n_runs; run += n_waves)" in src, name
        assert "render_grid(n_runs)" in src and "(size_t)n * kRenderRunsPerFrame" in src, name


def test_mono_chunk_equals_the_source():
    src = _text("iiv_mono.hip")
    assert int(_one(r"int chunk = chunk_env > 0 \? chunk_env : (\d+);", src)) == MB.CHUNK
    assert "f0 < n && !rc; f0 += chunk)" in src


def test_batch_sizes_reach_the_trips_and_the_chunk():
    assert (RB.N_SECOND, RB.N_THIRD) == (79, 157)
    for n in (RB.N_SECOND, RB.N_THIRD):
        RB.assert_trips(n)
    assert RB.trips(78) == 1 and RB.trips(79) == 2 and RB.trips(156) == 2 and RB.trips(157) == 3
    assert MB.N == 2051
    MB.assert_chunks(MB.N)


def _pairwise_different(a):
    flat = np.asarray(a).reshape(len(a), -1)
    return all((flat[i] != flat[j]).any() for i in range(len(a)) for j in range(i))


@pytest.mark.parametrize("mode", RB.MODES)
def test_render_pool_items_differ_in_every_expected_output(mode):
    assert RB.P == 7
    for pal_name in RB.PALETTES:
        rgb = RB.want_rgb(mode, pal_name)
        assert rgb.shape == (7, 192, 560, 3) and _pairwise_different(rgb), pal_name
        # ... in every one of the 105 runs of a frame: a single run taken from another item shows
        runs = rgb.reshape(7, RB.RUNS_PER_FRAME, -1)
        assert all((runs[i] != runs[j]).any(axis=1).all() for i in range(7) for j in range(i)), pal_name
    for pal_name in ("distinct", "NTSC"):
        for width in RB.WIDTHS:
            sums = RB.want_sums(mode, width, pal_name)
            assert sums.shape == (7, 3, 3) and sums.dtype == np.uint64
            for level in range(3):
                for ch in range(3):
                    assert len(set(sums[:, level, ch].tolist())) == 7, (pal_name, width, level, ch)
    own = RB.want_sums(mode, 560, "distinct", own=True)
    zero = np.isin(np.arange(7), RB.OWN)
    assert not own[zero].any() and own[~zero].all()
    assert (own[~zero] == RB.want_sums(mode, 560, "distinct")[~zero]).all()
    assert RB.STREAM0_ITEM % 7 != 0 and (RB.N_SECOND - 1) % 7 in RB.OWN


@pytest.mark.parametrize("mode", MB.MODES)
def test_mono_pool_items_differ_in_both_banks(mode):
    assert MB.P == 7 and len(MB.pool(mode)) == 7
    for dither in (M.DITHER_DIFFUSION, MB.ORDERED):
        main, aux = MB.want_maps(mode, dither)
        assert main.shape == (7, 32, 256) and _pairwise_different(main), dither
        assert (aux is None) == (mode == M.HGR)
        if aux is not None:
            assert _pairwise_different(aux), dither
        assert not (main == MB.FILL).any() and (aux is None or not (aux == MB.FILL).any())
    # and the two dithers give different maps: the neighbour case is not the loop's case again
    assert (MB.want_maps(mode, M.DITHER_DIFFUSION)[0] != MB.want_maps(mode, MB.ORDERED)[0]).any()
