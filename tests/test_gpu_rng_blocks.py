"""GPU: every kernel's MT19937 hand-over at every position of the 624-word block.

Five pieces of device code consume or advance the two Mersenne Twister streams of a clip (`random`: the three greedy kernels
-- iiv_workgroup.hip, iiv_greedy.hip in its LDS and its register form, iiv_team.h; `np.random`: iiv_prologue.hip), and each
crosses a block boundary in its own way.  Any 624 words with any index 0..624 are a legal state, so nothing here "advances" a
generator to a boundary: one batch holds the same block under EVERY index, and each stream is compared with the oracle started
from the same state -- opcodes, memory maps, priorities, draw counters and the final states of both generators in full (all
625 words of their canonical form, tests/mt_model.py: a wrong word deep in a written-back block fails here, not in whichever
later test happens to reach it).  What the sweeps cover is asserted from the oracle's own draw counts, so that a change of
content cannot lose a boundary case silently."""

import os
import random
import re

import numpy as np
import pytest

import encode_harness as H
import mt_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOLES = (np.arange(256) & 127) >= 120
PY_SEED, NP_SEED = 8128, 496


def _block(seed):
    """624 words of a real stream (the block random.seed(seed) leaves after 700 outputs)"""
    r = random.Random(seed)
    [r.getrandbits(32) for _ in range(700)]
    return np.array(r.getstate()[1][:624], dtype=np.uint32)


def _narrow(a):
    """a copy of `a` for the module-level caches, in 16 bits where that loses nothing (626 priority maps are 40 MiB as int32)"""
    a = np.asarray(a)
    return a.astype(np.uint16) if a.min() >= 0 and a.max() < 65536 else a.copy()


def _oracle_run(O, oracle_tables, mode, frames, sched, py_words, np_words, fourth=False):
    """One stream through the oracle from the given generator states, one opcode per call: everything a device stream is
    compared with, the draws of `random` per opcode and of `np.random` per restart."""
    v, ops, steps, seg_np = H.oracle_run(O, oracle_tables, mode, 5, frames, sched, (py_words, np_words), fourth=fourth, per_opcode=True)
    st = H.oracle_state(v, mode)
    st.up = [_narrow(u) for u in st.up]
    return {"ops": ops, "state": st, "draws": st.draws, "steps": steps, "seg_np": seg_np}


def _encoder(native, device_tables, mode, frames, py_states, np_states, kernel, fourth=False, prefix=True, dw=True):
    """An encoder of len(py_states) streams in the given generator states, and the target frames on the device.
    frames: (n_frames, 2, 32, 256), shared by all streams."""
    n = len(py_states)
    enc = H.make_encoder(native, device_tables, mode, 5, n, dw=dw, kernel=kernel, prefix=prefix, rng=list(zip(py_states, np_states)),
                         **({"fourth": True} if fourth else {}))
    fm, fa = H.device_frames(mode, [frames] * n)
    return enc, fm, fa


def _device_run(native, device_tables, mode, frames, sched, py_states, np_states, kernel, **options):
    enc, fm, fa = _encoder(native, device_tables, mode, frames, py_states, np_states, kernel, **options)
    ops = enc.encode(fm, fa, sched)
    enc.check()
    return enc, ops.cpu().numpy()


def _compare(native, enc, mode, ops, i, ref, tag):
    """opcodes and the whole state of stream i against its oracle run -> what was read from the device"""
    tag = "%s, stream %d" % (tag, i)
    H.check_ops(ops[i], ref["ops"], tag)
    return H.check_oracle_state(native, enc, i, ref["state"], mode, tag)


def _iid_frame(mode, seed):
    """one frame the way encode_harness.synth makes them"""
    return H.synth(mode, 1, seed)[0]


def _img_frame(mode, seed):
    """one picture-like frame (dithered bars: test_gpu_encode.test_image_like_streams' input)"""
    import stream_batch
    fm, fa = stream_batch.synth_frames_img(1, 1, mode == 1, seed=seed, device="cpu")
    fr = np.zeros((2, 32, 256), np.uint8)
    fr[0] = fm[0, 0].numpy()
    if mode == 1:
        fr[1] = fa[0, 0].numpy()
    return fr


# ---- a. `random`'s index sweep under every greedy form ------------------------------------------------------------------

# frame 0 picture-like, frame 1 iid.  A restart on each bank (HGR has one), every generator continued once (restart = 0),
# segments of one or two dozen opcodes: launches begin and end inside blocks, and the 626 oracle runs of a sweep stay cheap.
SWEEP_SCHED = {1: [(0, 0, 1, 24), (0, 0, 0, 13), (0, 1, 1, 24), (0, 1, 0, 7), (1, 0, 1, 20), (1, 0, 0, 11), (1, 1, 1, 17)],
               0: [(0, 0, 1, 24), (0, 0, 0, 13), (1, 0, 1, 20), (1, 0, 0, 11), (0, 0, 1, 17), (0, 0, 0, 7)]}
_SWEEP = {}


def _sweep_frames(mode):
    return np.stack([_img_frame(mode, 23), _iid_frame(mode, 4711)])


def _sweep_states():
    """streams 0..624: block B under index i; stream 625: (twist(B), 0), the same stream as 624.  One np.random state for all."""
    b = _block(PY_SEED)
    py = [mt_model.state(b, i) for i in range(625)] + [mt_model.state(mt_model.twist(b), 0)]
    npw = [mt_model.state(_block(NP_SEED), 100)] * 626
    return py, npw


def _sweep_oracle(O, oracle_tables, mode, fourth):
    """the oracle's 626 runs, once per (mode, fourth offset), shared by every kernel form"""
    if (mode, fourth) not in _SWEEP:
        frames = _sweep_frames(mode)
        py, npw = _sweep_states()
        refs = [_oracle_run(O, oracle_tables, mode, frames, SWEEP_SCHED[mode], py[i], npw[i], fourth) for i in range(626)]
        _sweep_coverage(refs, [int(s[624]) for s in py], SWEEP_SCHED[mode])
        _SWEEP[mode, fourth] = refs
    return _SWEEP[mode, fourth]


def _sweep_coverage(refs, start, sched):
    """What the sweep is for, from the oracle's draws per opcode.  Positions count words from the start of the block a stream
    starts in: draw number p is word p % 624 of block p // 624."""
    ends_on_623 = starts_on_0 = straddles_128 = launch_at_624 = 0
    seg_ends = np.cumsum([n for (_, _, _, n) in sched])[:-1]     # (a launch ends here and the next one begins)
    for ref, p0 in zip(refs, start):
        p = p0
        for k, d in enumerate(ref["steps"]):
            if d > 0:
                ends_on_623 += (p + d) % 624 == 0
                starts_on_0 += p % 624 == 0
                straddles_128 += d >= 128 and p // 624 != (p + d - 1) // 624
            p += d
            launch_at_624 += (k + 1) in seg_ends and p > 0 and p % 624 == 0
    assert ends_on_623 > 0, "no step's last draw is word 623"
    assert starts_on_0 > 0, "no step's first draw is word 0"
    assert straddles_128 > 0, "no step straddles a block boundary while drawing 128 words or more"
    assert launch_at_624 > 0, "no launch ends, and the next begins, with the index at exactly 624"
    return ends_on_623, starts_on_0, straddles_128, launch_at_624


@pytest.mark.parametrize("mode,kernel,fourth", [(m, k, f) for m in (1, 0) for f in (False, True)
                                                for k in ("plain", "shared", "team", False) if not (f and k is False)])
def test_random_index_sweep(native, O, oracle_tables, device_tables, mode, kernel, fourth):
    """626 streams, one launch sequence: the same frames, the same np.random state, `random`'s block B under index 0..624
    (stream i) and (twist(B), 0) (stream 625).  Every stream equals the oracle started from its state, and streams 624 and
    625 -- one stream under its two names -- equal each other.

    Which kernel a parameter reaches (iiv_encode.hip: launch_round; iiv_greedy.hip: launch_greedy_wave):
      "plain"   greedy_wave_kernel<MODE, 1, FOUR>: one wave per stream, the block and 256 words of the next in LDS
                (gen_ahead / move_head / gen_rest);
      "shared"  DHGR: greedy_wave_kernel<kDHGR, 8, FOUR>, the same LDS block per wave of a persistent workgroup;
                HGR: greedy_wave_kernel<kHGR, 16, FOUR>, the kMtRegs instantiation -- the block in registers (MtRegs), the
                queue of pending nonces, mt_behind; the only parameter that reaches it, with and without the fourth offset;
      "team"    iiv_team.h: the ring of kRing blocks, the MT wave twisting while the others score;
      False     iiv_workgroup.hip: two LDS blocks.  (With the fourth offset it runs the plain one-wave kernel
                -- include/iivision.h: IIV_OPT_FOURTH_OFFSET -- which "plain" already is: not repeated.)
    The fourth offset (one-wave kernel in both forms, team kernel) adds a third re-queued byte, so a third nonce behind the
    candidates', to a step."""
    refs = _sweep_oracle(O, oracle_tables, mode, fourth)
    py, npw = _sweep_states()
    enc, ops = _device_run(native, device_tables, mode, _sweep_frames(mode), SWEEP_SCHED[mode], py, npw, kernel, fourth=fourth)
    tag = "mode %d, kernel %r, fourth %r" % (mode, kernel, fourth)
    got = [_compare(native, enc, mode, ops, i, refs[i], tag) for i in range(626)]
    assert np.array_equal(ops[624], ops[625]), tag
    for b in range(mode + 1):
        assert np.array_equal(got[624]["mem"][b], got[625]["mem"][b]) and np.array_equal(got[624]["up"][b], got[625]["up"][b]), tag
    assert got[624]["draws"] == got[625]["draws"], tag
    H.same_stream(got[624]["py"], got[625]["py"], tag + ", streams 624 and 625, random")
    H.same_stream(got[624]["np"], got[625]["np"], tag + ", streams 624 and 625, np.random")
    enc.close()


# ---- b. one launch that draws more words than the team kernel's ring holds ------------------------------------------------

RING_STARTS = [0, 1, 311, 622, 623, 624, 227, 397]
RING_OPS = 300
_RING = {}


def _team_ring_blocks():
    """kRing of iiv_team.h, from its source: kRingNeed = (623 + kScorers * 258 + 2 + 623) / 624, kRing = kRingNeed + spare"""
    src = open(os.path.join(ROOT, "ii-vision_amd", "csrc", "iiv_team.h")).read()
    waves = re.search(r"constexpr int kScoringWaves = (\d+);", src)
    need = re.search(r"constexpr int kRingNeed = \(623 \+ kScorers \* 258 \+ 2 \+ 623\) / 624;", src)
    ring = re.search(r"constexpr int kRing = kRingNeed \+ (\d+);", src)
    assert waves and need and ring, "iiv_team.h no longer declares its ring the way this test reads it"
    return (623 + (int(waves.group(1)) - 1) * 258 + 2 + 623) // 624 + int(ring.group(1))


def _ring_oracle(O, oracle_tables, mode, content):
    if (mode, content) not in _RING:
        frames = (_iid_frame(mode, 1234) if content == "iid" else _img_frame(mode, 5))[None]
        b, npw = _block(PY_SEED + 1), mt_model.state(_block(NP_SEED + 1), 7)
        py = [mt_model.state(b, i) for i in RING_STARTS]
        refs = [_oracle_run(O, oracle_tables, mode, frames, [(0, 0, 1, RING_OPS)], s, npw) for s in py]
        _RING[mode, content] = (frames, py, [npw] * len(py), refs)
    return _RING[mode, content]


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("content", ["iid", "img"])
@pytest.mark.parametrize("kernel", ["team", "plain", "shared"])
def test_launch_past_the_team_ring(native, O, oracle_tables, device_tables, mode, content, kernel):
    """One launch whose draws of `random` exceed the kRing blocks the team kernel keeps in LDS: every ring slot is dropped,
    refilled and read again (ring_drop, the MT wave's growth, ring_word's block arithmetic at every block of a round).  Under
    the one-wave forms the same launch moves the LDS head, or the registers behind their queue, through as many blocks.
    Eight start indices; iid content, and picture-like content besides: on iid input a step's winners hardly ever hang on a
    nonce, so a wrong word shows in the final state only -- on picture-like input it changes the opcodes."""
    frames, py, npw, refs = _ring_oracle(O, oracle_tables, mode, content)
    ring_words = _team_ring_blocks() * 624
    for ref in refs:
        assert ref["draws"][0] > ring_words, "the launch draws %d words, the ring holds %d" % (ref["draws"][0], ring_words)
    enc, ops = _device_run(native, device_tables, mode, frames, [(0, 0, 1, RING_OPS)], py, npw, kernel)
    for i in range(len(py)):
        _compare(native, enc, mode, ops, i, refs[i], "mode %d, %s, kernel %r, start index %d" % (mode, content, kernel, RING_STARTS[i]))
    enc.close()


# ---- c. np.random's index sweep in the prologue --------------------------------------------------------------------------

_PRO = {}
PRO_TARGETS = ("blank", "few", "constant")


def _pro_frames(mode):
    """frame 0: blank; 1: forty bytes that differ from the blank screen; 2: test_constant_target_degenerate_priorities' target"""
    fr = np.zeros((3, 2, 32, 256), np.uint8)
    rng = np.random.default_rng(77)
    for b in range(mode + 1):
        idx = rng.choice(np.nonzero(~np.tile(HOLES, 32))[0], 40, replace=False)
        fr[1, b].reshape(-1)[idx] = rng.integers(1, 128, 40)
    fr[2, 0], fr[2, 1] = 0x55, 0x2A
    fr[2][..., HOLES] = 0
    return fr


def _pro_sched(mode, target):
    """every generator pulled for one opcode: the prologue is what runs.  DHGR: a restart on each bank; HGR: two on its one --
    the second prologue starts from wherever the first left the index, and the first has a known budget (IIV_OPT_PREFIX_SORT)"""
    f = PRO_TARGETS.index(target)
    return [(f, 0, 1, 1), (f, 1 if mode == 1 else 0, 1, 1)]


def _pro_states():
    b = _block(NP_SEED + 2)
    return [mt_model.state(_block(PY_SEED + 2), 100)] * 625, [mt_model.state(b, i) for i in range(625)]


def _pro_oracle(O, oracle_tables, mode, target):
    if (mode, target) not in _PRO:
        py, npw = _pro_states()
        refs = [_oracle_run(O, oracle_tables, mode, _pro_frames(mode), _pro_sched(mode, target), py[i], npw[i]) for i in range(625)]
        n = refs[0]["seg_np"][0]       # the first prologue's draws: one per byte with a non-zero priority, whatever the nonces
        assert all(r["seg_np"][0] == n for r in refs)
        ends = np.arange(625) + n      # first + n of stream i
        if target == "blank":
            assert n == 0 and all(r["draws"] == (0, 0) for r in refs)
        elif target == "few":
            assert 0 < n < 624
            assert (ends < 624).any() and (ends > 624).any() and (ends == 624).sum() == 1
        else:
            assert n == 7680
            # iiv_prologue.hip generates (first + 7679) / 624 blocks ahead: 12 and 13 inside the sweep; one stream ends a block
            assert set(((np.arange(625) + 7679) // 624).tolist()) == {12, 13}
            assert (ends % 624 == 0).sum() == 1
        _PRO[mode, target] = refs
    return _PRO[mode, target]


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("target", PRO_TARGETS)
@pytest.mark.parametrize("prefix,dw", [(True, True), (False, True), (True, "table"), (True, "split")])
def test_np_random_index_sweep_in_the_prologue(native, O, oracle_tables, device_tables, mode, target, prefix, dw):
    """625 streams, np.random's block under index 0..624, one `random` state; three targets on a blank screen: nothing to draw
    (the state comes back bit for bit, index included), a few dozen draws (first + n below, at and beyond 624 within the
    sweep), and 7680, the most a prologue draws (twelve or thirteen blocks generated ahead; first + n a multiple of 624 for one
    stream).  dw: IIV_OPT_DIFF_WEIGHTS selects the prologue_kernel<MODE, DP> instantiation -- one run of each."""
    refs = _pro_oracle(O, oracle_tables, mode, target)
    py, npw = _pro_states()
    enc, ops = _device_run(native, device_tables, mode, _pro_frames(mode), _pro_sched(mode, target), py, npw, "plain",
                           prefix=prefix, dw=dw)
    tag = "mode %d, target %s, prefix sort %r, diff weights %r" % (mode, target, prefix, dw)
    for i in range(625):
        st = _compare(native, enc, mode, ops, i, refs[i], tag)
        if target == "blank":
            assert np.array_equal(st["np"], npw[i]), "%s, stream %d: np.random's state moved without a draw" % (tag, i)
            assert np.array_equal(st["py"], py[i]), "%s, stream %d: random's state moved without a draw" % (tag, i)
            assert st["draws"] == (0, 0)
            assert (ops[i][:, 0] == 32).all() and (ops[i][:, 1:] == 0).all()
    enc.close()


# ---- d. snapshot and rollback across a boundary --------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["team", "plain"])
def test_snapshot_and_rollback_across_a_boundary(native, O, oracle_tables, device_tables, kernel):
    """A snapshot in slot 1 with both generators at index 623, an encode across the boundary (prologue and greedy launches),
    the rollback, the same encode again: the same opcodes and the same streams as the first time and as the oracle's straight run."""
    mode = 1
    frames = _sweep_frames(mode)
    sched = [(0, 0, 1, 30), (0, 0, 0, 10), (1, 1, 1, 25)]
    py, npw = [mt_model.state(_block(PY_SEED + 3), 623)], [mt_model.state(_block(NP_SEED + 3), 623)]
    ref = _oracle_run(O, oracle_tables, mode, frames, sched, py[0], npw[0])
    assert ref["draws"][0] > 1 and ref["draws"][1] > 1       # (both streams cross)
    enc, fm, fa = _encoder(native, device_tables, mode, frames, py, npw, kernel)
    enc.snapshot(1)
    runs = []
    for again in (False, True):
        if again:
            enc.rollback(1)
            assert np.array_equal(enc.get_state(native.STATE_RNG_PY), py[0]) and np.array_equal(enc.get_state(native.STATE_RNG_NP), npw[0])
            assert enc.get_state(native.STATE_COUNTERS)[:2].tolist() == [0, 0]
        ops = enc.encode(fm, fa, sched).cpu().numpy()
        enc.check()
        runs.append((ops, _compare(native, enc, mode, ops, 0, ref, "kernel %r, %s" % (kernel, "after the rollback" if again else "first run"))))
    assert np.array_equal(runs[0][0], runs[1][0])
    H.same_stream(runs[1][1]["py"], runs[0][1]["py"], "random, second run against the first")
    H.same_stream(runs[1][1]["np"], runs[0][1]["np"], "np.random, second run against the first")
    enc.close()
