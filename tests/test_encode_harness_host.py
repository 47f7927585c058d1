"""CPU: the shared checks of tests/encode_harness.py cannot pass blindly.  A stand-in for the encoder answers get_state from
arrays filled from a short oracle run; untouched it passes both state checkers, and one changed value in any compared field
makes the checker raise and name the field.  The same for check_ops, for the aux bank's absence in HGR, and for the bytes
synth() hands every oracle expectation."""
import hashlib

import numpy as np
import pytest

import encode_harness as H

DHGR, HGR = 1, 0
N_OPS = 40


@pytest.fixture(scope="module")
def native():
    import _iiv_native          # (the STATE_* constants only: the library is not loaded)
    return _iiv_native


class StandIn:
    """enc.get_state(what, i) over a copy of an oracle_state; `reads` lists what was asked for"""

    def __init__(self, native, st, ops):
        n = native
        self.items = {n.STATE_PACKED: st.packed.copy(), n.STATE_OUT_OF_WORK: np.array(st.out_of_work, np.int32),
                      n.STATE_COUNTERS: np.array(list(st.draws) + [len(ops), 0], np.uint64),
                      n.STATE_RNG_PY: st.py.copy(), n.STATE_RNG_NP: st.np.copy()}
        for b in range(len(st.mem)):
            self.items[n.STATE_MEM_MAIN + b] = st.mem[b].copy()
            self.items[n.STATE_UP_MAIN + b] = st.up[b].astype(np.int32)
        self.reads = []

    def get_state(self, what, stream=0):
        self.reads.append(what)
        return self.items[what].copy()


def _run(O, oracle_tables, mode):
    sched = [(0, 0, N_OPS), (0, 1 if mode == DHGR else 0, N_OPS)]
    v, ops = H.oracle_run(O, oracle_tables, mode, 5, H.synth(mode, 1, 606), sched, (61, 62))
    return H.oracle_state(v, mode), ops


def _record(O, mode, st, ops):
    rec = {"meta": np.array([mode, 5, 61, 62]), "ops": ops, "mem_main": st.mem[0], "up_main": st.up[0], "packed": st.packed,
           "out_of_work": np.array(st.out_of_work), "py_next": np.array(H.next_draws(O, st.py, 4, True)),
           "np_next": np.array(H.next_draws(O, st.np, 4, False))}
    if mode == DHGR:
        rec.update(mem_aux=st.mem[1], up_aux=st.up[1])
    return rec


@pytest.fixture(scope="module")
def dhgr(O, oracle_tables):
    st, ops = _run(O, oracle_tables, DHGR)
    return st, ops, _record(O, DHGR, st, ops)


def test_the_run_moves_every_compared_field(O, dhgr):
    """DHGR, one frame, 40 opcodes on each bank: both banks' memory and priorities, the packed screen and both generators
    have all moved off their initial values -- a checker that compared nothing would not be told apart otherwise"""
    st, ops, _ = dhgr
    assert len(ops) == 2 * N_OPS
    for b in (0, 1):
        assert st.mem[b].any() and st.up[b].any(), b
    assert st.packed.any()
    assert st.draws[0] > 0 and st.draws[1] > 0
    fresh = H.seed_states(O, 61, 62)
    assert not np.array_equal(st.py, fresh[0]) and not np.array_equal(st.np, fresh[1])
    assert st.py[624] < 620 and st.np[624] < 620      # (the four next draws of each lie in the block at hand)


def test_the_untouched_stand_in_passes(native, O, dhgr):
    st, ops, rec = dhgr
    enc = StandIn(native, st, ops)
    got = H.check_oracle_state(native, enc, 0, st, DHGR, "untouched")
    assert sorted(got) == sorted(H.FIELDS)
    H.check_recorded_state(native, O, enc, 0, rec, "untouched")
    H.check_ops(ops.copy(), ops, "untouched")


def _index_moved(words):
    words[624] += 1


def _word_flipped(words):
    words[int(words[624])] ^= np.uint32(0xFFFFFFFF)     # the next word to be drawn: tempered, the draw's eight bits change too


# (what to change in the stand-in, how, the field's name in check_oracle_state's message, in check_recorded_state's or None)
FLIPS = [
    ("STATE_MEM_MAIN", lambda a: a.__setitem__((3, 5), a[3, 5] ^ 1), "mem of bank 0", "mem_main"),
    ("STATE_MEM_AUX", lambda a: a.__setitem__((31, 119), a[31, 119] ^ 0x40), "mem of bank 1", "mem_aux"),
    ("STATE_UP_MAIN", lambda a: a.__setitem__((0, 0), a[0, 0] + 1), "up of bank 0", "up_main"),
    ("STATE_UP_AUX", lambda a: a.__setitem__((17, 64), a[17, 64] + 65536), "up of bank 1", "up_aux"),
    ("STATE_PACKED", lambda a: a.__setitem__((9, 100), a[9, 100] ^ np.uint64(1 << 40)), "packed", "packed"),
    ("STATE_OUT_OF_WORK", lambda a: a.__setitem__(0, 1 - a[0]), "out_of_work", "out_of_work"),
    ("STATE_OUT_OF_WORK", lambda a: a.__setitem__(1, 1 - a[1]), "out_of_work", "out_of_work"),
    ("STATE_COUNTERS", lambda a: a.__setitem__(0, a[0] + np.uint64(1)), "draws", None),
    ("STATE_COUNTERS", lambda a: a.__setitem__(1, a[1] + np.uint64(1)), "draws", None),
    ("STATE_RNG_PY", _word_flipped, "py (random)", "py_next"),
    ("STATE_RNG_NP", _word_flipped, "np (np.random)", "np_next"),
    ("STATE_RNG_PY", _index_moved, "py (random)", "py_next"),
    ("STATE_RNG_NP", _index_moved, "np (np.random)", "np_next"),
]


@pytest.mark.parametrize("k", range(len(FLIPS)))
def test_one_changed_value_fails_and_names_the_field(native, O, dhgr, k):
    st, ops, rec = dhgr
    what, change, named, recorded_as = FLIPS[k]
    enc = StandIn(native, st, ops)
    before = enc.items[getattr(native, what)].copy()
    change(enc.items[getattr(native, what)])
    assert (enc.items[getattr(native, what)] != before).sum() == 1       # a single value
    with pytest.raises(AssertionError) as e:
        H.check_oracle_state(native, enc, 0, st, DHGR, "flip")
    assert named in str(e.value), str(e.value)
    if recorded_as is not None:      # (a recording holds no draw counters)
        with pytest.raises(AssertionError) as e:
            H.check_recorded_state(native, O, enc, 0, rec, "flip")
        assert recorded_as in str(e.value), str(e.value)
    # the subset a call site may name leaves the other fields out, and only those
    others = tuple(f for f in H.FIELDS if f != named.split()[0])
    H.check_oracle_state(native, enc, 0, st, DHGR, "flip", fields=others)


def test_raw_index_624_is_index_0_of_the_next_block(native, dhgr):
    """(B, 624) and (twist(B), 0) are one stream: no difference to check_oracle_state"""
    import mt_model
    st, ops, _ = dhgr
    enc = StandIn(native, st, ops)
    block = st.py[:624].copy()
    enc.items[native.STATE_RNG_PY] = mt_model.state(block, 624)
    want = H.State(**{**vars(st), "py": mt_model.state(mt_model.twist(block), 0)})
    H.check_oracle_state(native, enc, 0, want, DHGR, "624")
    want.py = mt_model.state(block, 0)
    with pytest.raises(AssertionError):
        H.check_oracle_state(native, enc, 0, want, DHGR, "624")


def test_check_ops_sees_the_first_row_the_last_row_and_a_short_count(dhgr):
    _, ops, _ = dhgr
    for row in (0, len(ops) - 1):
        got = ops.copy()
        got[row, 3] ^= 1
        with pytest.raises(AssertionError) as e:
            H.check_ops(got, ops, "flip")
        assert "mismatch at %d " % row in str(e.value)
    with pytest.raises(AssertionError) as e:
        H.check_ops(ops[:-1], ops, "short")
    assert "shape" in str(e.value)


def test_hgr_reads_no_aux_field(native, O, oracle_tables):
    """HGR: the stand-in has no aux items and the record no aux keys -- reading either would be a KeyError"""
    st, ops = _run(O, oracle_tables, HGR)
    assert len(st.mem) == 1 and st.mem[0].any() and st.draws[0] > 0
    enc = StandIn(native, st, ops)
    assert native.STATE_MEM_AUX not in enc.items and native.STATE_UP_AUX not in enc.items
    H.check_oracle_state(native, enc, 0, st, HGR, "hgr")
    H.check_recorded_state(native, O, enc, 0, _record(O, HGR, st, ops), "hgr")
    assert native.STATE_MEM_AUX not in enc.reads and native.STATE_UP_AUX not in enc.reads
    assert native.STATE_MEM_MAIN in enc.reads and native.STATE_RNG_NP in enc.reads


# sha256 of synth(mode, n_frames, seed, coherent), computed from test_gpu_encode._synth before it moved here:
# stream 0 and stream 1 of test_batch_of_independent_streams (DHGR), test_generator_advanced_a_few_opcodes_per_launch (HGR)
SYNTH = [((1, 3, 100, False), "438289ff3717069eb3c189471456089d6326d46440c5b1f2eda252ad16c03927"),
         ((1, 3, 101, True), "f40409a21489aeb4d2380a2c8aca59de138862181eb37a632dafab52ec4a88c7"),
         ((0, 2, 4246, True), "287fda31fc8b1a190086470f644c1a127b0f0f7927165e36309fe473c66974cb")]


@pytest.mark.parametrize("args,digest", SYNTH)
def test_synth_is_byte_identical(args, digest):
    assert hashlib.sha256(H.synth(*args).tobytes()).hexdigest() == digest
