"""CPU: what tests/test_gpu_speaker_batches.py relies on without being able to see it.

  the constants   kSpeakerRun, kSpeakerGridCap, the block size and the samples per thread are read from the text of
                  csrc/iiv_speaker.hip and must equal what tests/speaker_cases.py mirrors: a changed cap fails here, instead of
                  passing unnoticed while the GPU test silently stops reaching the loop
  the arithmetic  1025 rows of 2040 opcodes are the least with a second trip at decim 73, 2049 with a third
  the pool        on the model alone: the seven items' expected rows are pairwise different, so "another row's samples" can never
                  equal the right ones"""
import os
import re

import pytest

import speaker_cases as SC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ii-vision_amd", "csrc")


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_speaker_constants_equal_the_source():
    with open(os.path.join(CSRC, "iiv_speaker.hip")) as f:
        src = f.read()
    assert int(_one(r"constexpr int kSpeakerRun = (\d+);", src)) == SC.RUN
    assert int(_one(r"constexpr int kSpeakerGridCap = (\d+);", src)) == SC.GRID_CAP
    assert int(_one(r"constexpr int kSpeakerThreads = (\d+);", src)) == SC.THREADS
    assert int(_one(r"constexpr int kSpeakerPerThread = (\d+);", src)) == SC.PER_THREAD
    assert SC.RUN == SC.THREADS * SC.PER_THREAD
    # the list of items is streams times runs, the grid is capped, and the loop strides by the grid
    assert "const size_t runs = ((size_t)m_max + kSpeakerRun - 1) / kSpeakerRun;" in src
    assert "const size_t n_items = (size_t)n_streams * runs;" in src
    assert "(unsigned)(n_items < (size_t)kSpeakerGridCap ? n_items : (size_t)kSpeakerGridCap)" in src
    assert "for (size_t item = blockIdx.x; item < n_items; item += gridDim.x)" in src


def test_batch_sizes_reach_the_trips():
    assert (SC.N_SECOND, SC.N_THIRD) == (1025, 2049)
    for n in (SC.N_SECOND, SC.N_THIRD):
        SC.assert_trips(n)


@pytest.mark.parametrize("order,gain", [(1, 73), (3, 16384), (4, 32767)])
def test_pool_rows_differ(order, gain):
    want = SC.pool_want(order, gain)
    assert want.shape == (7, 2052)
    for i in range(7):
        for j in range(i):
            assert (want[i] != want[j]).any(), (i, j)
            # ... in the first run and, where both have one, in the second
            assert (want[i, :SC.RUN] != want[j, :SC.RUN]).any(), (i, j)
    assert (want[4] == SC.SENTINEL).all() and (want[3, 302:] == SC.SENTINEL).all() and (want[3, :302] != SC.SENTINEL).all()
