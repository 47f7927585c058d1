"""CPU: tests/mt_model.py against the three MT19937 implementations the GPU tests lean on -- CPython's `random`, numpy's
`RandomState` and the oracle's -- started INSIDE a block: every start index at which one of the twist's three thirds begins
or ends (227, 454: the word a new word is built from changes from old to new; 397: word i + 397 wraps), the block's two
ends, and 1300 draws, so that every start crosses two block boundaries."""

import ctypes as C
import random

import numpy as np
import pytest

import mt_model

INDICES = [0, 1, 226, 227, 228, 396, 397, 398, 453, 454, 455, 622, 623, 624]
SEEDS = [1, 5489, 20240229]
N_DRAWS = 1300


def _block(seed):
    """624 words of a real stream: the block `random.seed(seed)` leaves after a few hundred draws (not the seeding pattern)"""
    r = random.Random(seed)
    [r.getrandbits(32) for _ in range(700)]
    return np.array(r.getstate()[1][:624], dtype=np.uint32)


@pytest.fixture(scope="module")
def model_draws():
    """(seed, index) -> (the model's next N_DRAWS getrandbits(8), its next N_DRAWS randint(0, 256)); computed once"""
    out = {}
    for seed in SEEDS:
        b = _block(seed)
        for idx in INDICES:
            sp, sn = mt_model.state(b, idx), mt_model.state(b, idx)
            out[seed, idx] = ([mt_model.draw_py(sp) for _ in range(N_DRAWS)], [mt_model.draw_np(sn) for _ in range(N_DRAWS)])
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_model_equals_python_random(model_draws, seed):
    saved = random.getstate()
    try:
        b = _block(seed)
        for idx in INDICES:
            random.setstate((3, tuple(int(w) for w in b) + (idx,), None))
            assert [random.getrandbits(8) for _ in range(N_DRAWS)] == model_draws[seed, idx][0], idx
    finally:
        random.setstate(saved)


@pytest.mark.parametrize("seed", SEEDS)
def test_model_equals_numpy_randomstate(model_draws, seed):
    saved = np.random.get_state()
    try:
        b = _block(seed)
        for idx in INDICES:
            rs = np.random.RandomState()
            rs.set_state(("MT19937", b, idx))
            assert [int(rs.randint(0, 256)) for _ in range(N_DRAWS)] == model_draws[seed, idx][1], idx
            # ... and the global generator the reference draws from (video.py:265)
            np.random.set_state(("MT19937", b, idx))
            assert np.random.randint(0, 256, size=N_DRAWS).tolist() == model_draws[seed, idx][1], idx
    finally:
        np.random.set_state(saved)


@pytest.mark.parametrize("seed", SEEDS)
def test_model_equals_oracle(O, model_draws, seed):
    L = O.lib()
    b = _block(seed)
    for idx in INDICES:
        for f, want in ((L.orc_py_getrandbits8, model_draws[seed, idx][0]), (L.orc_np_randint256, model_draws[seed, idx][1])):
            m = O.MT()
            m.set_state_words(mt_model.state(b, idx))
            assert [f(C.byref(m)) for _ in range(N_DRAWS)] == want, idx


def test_twist_is_the_generators_block_update():
    """twist() by itself: the block a generator holds after crossing a boundary, word for word"""
    saved = random.getstate()
    try:
        for seed in SEEDS:
            b = _block(seed)
            random.setstate((3, tuple(int(w) for w in b) + (624,), None))
            random.getrandbits(32)
            got = random.getstate()[1]
            assert got[624] == 1 and np.array_equal(np.array(got[:624], dtype=np.uint32), mt_model.twist(b))
    finally:
        random.setstate(saved)


def test_canonical():
    """(B, 624) and (twist(B), 0) are one stream and one canonical form; every other index is its own"""
    for seed in SEEDS:
        b = _block(seed)
        at_end, at_start = mt_model.state(b, 624), mt_model.state(mt_model.twist(b), 0)
        assert not np.array_equal(at_end, at_start)
        assert np.array_equal(mt_model.canonical(at_end), mt_model.canonical(at_start))
        assert np.array_equal(mt_model.canonical(at_start), at_start)
        for draw in (mt_model.draw_py, mt_model.draw_np):
            a, c = at_end.copy(), at_start.copy()
            assert [draw(a) for _ in range(N_DRAWS)] == [draw(c) for _ in range(N_DRAWS)]
            assert np.array_equal(a, c)      # (past the first draw the two are the same words and index)
        for idx in (0, 1, 397, 623):
            s = mt_model.state(b, idx)
            assert np.array_equal(mt_model.canonical(s), s)
        assert not np.array_equal(mt_model.canonical(mt_model.state(b, 623)), mt_model.canonical(at_end))
    before = mt_model.state(_block(1), 624)
    keep = before.copy()
    mt_model.canonical(before)
    assert np.array_equal(before, keep)      # (canonical() copies)


def test_team_ring_word_division_is_exact():
    """iiv_team.h: ring_word finds the block of stream word q as (q * MUL) >> SHIFT instead of q / 624.  That is exact only
    up to some q; it has to be exact for every word a round can read, the bound the header's own static_assert states
    (623 + kScorers * 258 + 2).  Read from the source, so that a change of the multiplier, the shift, the number of scoring
    waves or the bound is held to the arithmetic here, without a GPU."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ii-vision_amd", "csrc", "iiv_team.h")).read()
    mul = re.search(r"const int b = \(int\)\(\(\(uint32_t\)q \* (\d+)u\) >> (\d+)\);", src)
    waves = re.search(r"constexpr int kScoringWaves = (\d+);", src)
    bound = re.search(r"static_assert\(623 \+ kScorers \* 258 \+ 2 <= (\d+),", src)
    assert mul and waves and bound, "iiv_team.h no longer states ring_word's division the way this test reads it"
    m, sh, limit = int(mul.group(1)), int(mul.group(2)), int(bound.group(1))
    reach = 623 + (int(waves.group(1)) - 1) * 258 + 2
    assert reach <= limit
    q = np.arange(limit, dtype=np.int64)
    assert np.array_equal((q * m) >> sh, q // 624), "ring_word's block index is wrong below the bound the header asserts"
    assert limit * m < 1 << 32      # (the product is formed in 32 bits)
