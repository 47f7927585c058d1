"""CPU: the clips of tests/assert_inputs.py do what they are for -- shown with the oracle alone -- and on them the oracle
equals the reference, whose runs tests/golden/make_golden.py --asserts-only recorded in tests/golden/g10_asserts.npz: the
opcodes (for the asserting clips: the ones yielded before the AssertionError, and the line that raised), the final memory
maps and priorities, and the next four draws of both generators.  tests/test_gpu_reference_asserts.py then holds every
kernel form to the oracle on the same inputs.  Every comparison is exact."""
import hashlib
import os

import numpy as np
import pytest

import assert_inputs as A

_G10 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_asserts.npz")


@pytest.fixture(scope="module")
def g10():
    return np.load(_G10)


def _table(oracle_tables, mode):
    return oracle_tables.get(mode, 5)


@pytest.mark.parametrize("mode", A.MODES)
def test_dirty_holes_runs_clean_and_the_hole_bytes_matter(O, oracle_tables, mode):
    frames, sched = A.dirty_holes(mode), A.dirty_holes_schedule(mode)
    assert frames.shape == (3, 2, 32, 256) and sum(g[3] for g in sched) == 600
    used = frames[:, :mode + 1]
    assert (used[..., A.HOLES] != 0).all()
    if mode == A.DHGR:
        assert (used[..., ~A.HOLES] < 0x80).all()
        share = (used[..., A.HOLES] >= 0x80).mean()
        assert 0.4 < share < 0.6
    low = used & (0x7f if mode == A.DHGR else 0xff)
    cols = A.HOLES | A.HOLE_NEIGHBOURS
    assert (low[1:][..., cols] != low[:-1][..., cols]).all()                # scored in every generator, from black too:
    assert (low[0][..., cols] != 0).all()
    v, ops, code = A.oracle_run(O, mode, _table(oracle_tables, mode), frames, sched, A.SEEDS["dirty_holes"])
    assert code == 0 and len(ops) == 600
    tidy = A.dirty_holes(mode, tidy=True)
    assert (tidy[..., A.HOLES] == 0).all() and np.array_equal(tidy[..., ~A.HOLES], frames[..., ~A.HOLES])
    _, ops_tidy, code = A.oracle_run(O, mode, _table(oracle_tables, mode), tidy, sched, A.SEEDS["dirty_holes"])
    assert code == 0
    first = np.nonzero((ops != ops_tidy).any(axis=1))[0]
    assert len(first) and first[0] < 150                                    # already within the first generator
    assert all((v.memory(b)[:, A.HOLES] == 0).all() for b in A.banks(mode))  # (nothing is ever stored into a hole)


def test_quiet_palette_bit_runs_clean(O, oracle_tables):
    table = _table(oracle_tables, A.DHGR)
    frames, sched = A.quiet_palette_bit(O, table)
    n_quiet = [(frames[f, b] >= 0x80).sum() for f in range(2) for b in range(2)]
    assert min(n_quiet) > 1000 and (frames[0, 0] == 0x80).sum() > 1000       # 0x80 in the black parts of the first target
    assert (frames[0, 0] & 0x7f != 0).sum() > 1000                           # ... of a picture that is being drawn
    assert (frames[..., A.HOLES] == 0).all()
    v, ops, code = A.oracle_run(O, A.DHGR, table, frames, sched, A.SEEDS["quiet"])
    assert code == 0 and len(ops) == 600 and (ops[:, 1] < 0x80).all()
    # the same bytes WOULD assert if one of them were popped: with bit 7 on a byte that is drawn, the oracle stops
    loud = frames.copy()
    page, off = ops[0, 0] - 32, ops[0, 2]
    loud[0, 0, page, off] |= 0x80
    _, ops2, code = A.oracle_run(O, A.DHGR, table, loud, sched, A.SEEDS["quiet"])
    assert code == A.ERR_PALETTE_BIT and len(ops2) == 0


def test_late_palette_bit_asserts_in_the_continuation_only(O, oracle_tables):
    table = _table(oracle_tables, A.DHGR)
    frames = A.late_palette_bit()
    assert (frames >= 0x80).sum() == 1 and frames[0, 0, A.LATE_AT[0], A.LATE_AT[1]] == 0x81
    v, ops, code = A.oracle_run(O, A.DHGR, table, frames, A.LATE_SHORT, A.SEEDS["late"])
    assert code == 0 and len(ops) == sum(g[3] for g in A.LATE_SHORT)
    assert v.update_priority(0)[A.LATE_AT] > 0                                # still waiting
    _, more, code = A.oracle_run(O, A.DHGR, table, frames, A.LATE_MORE, A.SEEDS["late"], v=v)
    assert code == A.ERR_PALETTE_BIT and len(more) == A.LATE_MORE_INDEX > 0
    assert A.LATE_MORE_INDEX < A.LATE_MORE[0][3] and A.LATE_SHORT[-1][3] + A.LATE_MORE_INDEX == A.LATE_INDEX


def test_early_palette_bit_asserts_in_the_first_launch(O, oracle_tables):
    frames = A.early_palette_bit()
    assert (frames[0, 0] >= 0x80).sum(axis=1).tolist() == [2] * 32 and (frames[1:] < 0x80).all() and (frames[0, 1] < 0x80).all()
    _, ops, code = A.oracle_run(O, A.DHGR, _table(oracle_tables, A.DHGR), frames, A.EARLY_SCHEDULE, A.SEEDS["early"])
    assert code == A.ERR_PALETTE_BIT and 1 <= len(ops) <= 199


def test_clean_clips_run_clean(O, oracle_tables):
    for mode in A.MODES:
        for name in ("clean", "clean2"):
            first, second = A.clean_schedules(mode)
            _, ops, code = A.oracle_run(O, mode, _table(oracle_tables, mode), A.clean(mode, name), first + second, A.SEEDS[name])
            assert code == 0 and len(ops) == 600


def _cases(O, oracle_tables):
    quiet, quiet_sched = A.quiet_palette_bit(O, _table(oracle_tables, A.DHGR))
    return [("dirty_holes_DHGR", A.DHGR, A.dirty_holes(A.DHGR), A.dirty_holes_schedule(A.DHGR), "dirty_holes", 0),
            ("dirty_holes_HGR", A.HGR, A.dirty_holes(A.HGR), A.dirty_holes_schedule(A.HGR), "dirty_holes", 0),
            ("quiet", A.DHGR, quiet, quiet_sched, "quiet", 0),
            ("late_short", A.DHGR, A.late_palette_bit(), A.LATE_SHORT, "late", 0),
            ("late_more", A.DHGR, A.late_palette_bit(), A.LATE_SHORT + A.LATE_MORE, "late", 137),
            ("early", A.DHGR, A.early_palette_bit(), A.EARLY_SCHEDULE, "early", 137)]


def test_oracle_equals_the_reference_on_these_inputs(O, oracle_tables, g10):
    """the reference's own run of every clip: opcodes up to its AssertionError, the line that raised, the state it left"""
    for (tag, mode, frames, sched, seeds, line) in _cases(O, oracle_tables):
        g = lambda k: g10[tag + "/" + k]
        # the clip and schedule the reference ran are the ones this module builds
        assert hashlib.sha256(np.ascontiguousarray(frames).tobytes()).digest() == g("sha_frames").tobytes(), tag
        assert g("schedule").tolist() == [list(s) for s in sched], tag
        assert int(g("assert_line")) == line, tag
        v, ops, code = A.oracle_run(O, mode, _table(oracle_tables, mode), frames, sched, A.SEEDS[seeds])
        assert code == (A.ERR_PALETTE_BIT if line else 0), tag
        assert int(g("n_ops")) == len(ops) and np.array_equal(ops, g("ops")), tag
        if not line:
            assert len(ops) == sum(s[3] for s in sched), tag
        assert np.array_equal(v.memory(0), g("mem_main")) and np.array_equal(v.update_priority(0), g("up_main")), tag
        assert np.array_equal(v.packed, g("packed")), tag
        if mode == A.DHGR:
            assert np.array_equal(v.memory(1), g("mem_aux")) and np.array_equal(v.update_priority(1), g("up_aux")), tag
        assert A.next_draws(O, v.rng_py().state_words(), True) == g("py_next").tolist(), tag
        assert A.next_draws(O, v.rng_np().state_words(), False) == g("np_next").tolist(), tag
