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
    v = O.Video(mode, oracle_tables.get(mode, 5))
    v.rng_py().set_state_words(py_words)     # (the generators live inside the oracle's Video: orc_video_rng_py / _np)
    v.rng_np().set_state_words(np_words)
    v.set_fourth_offset(fourth)
    ops, steps, seg_np = [], [], []
    for (f, ia, restart, n) in sched:
        if restart:
            before = v.draws()[1]
            v.encode_frame(frames[f, 0], frames[f, 1] if mode == 1 else None, ia)
        for k in range(n):
            d0 = v.draws()[0]
            ops.append(v.next(1))
            if restart and k == 0:
                seg_np.append(v.draws()[1] - before)     # (the reference's generator is lazy: its prologue runs in the first next())
            steps.append(v.draws()[0] - d0)
    return {"ops": np.concatenate(ops), "mem": [v.memory(b).copy() for b in range(mode + 1)],
            "up": [_narrow(v.update_priority(b)) for b in range(mode + 1)], "draws": v.draws(),
            "py": v.rng_py().state_words(), "np": v.rng_np().state_words(), "steps": steps, "seg_np": seg_np}


def _encoder(native, device_tables, mode, frames, py_states, np_states, kernel, fourth=False, prefix=True, dw=True):
    """An encoder of len(py_states) streams in the given generator states, and the target frames on the device.
    frames: (n_frames, 2, 32, 256), shared by all streams."""
    import torch
    n = len(py_states)
    t, s = device_tables.get(mode, 5)
    enc = native.Encoder(mode, t, s, n, dm=device_tables.dm[(mode, 5)])
    enc.set_diff_weights_mode(dw)
    enc.set_greedy_kernel(kernel)
    enc.set_prefix_sort(prefix)
    if fourth:
        enc.set_fourth_offset(True)
    fr = torch.from_numpy(np.ascontiguousarray(frames)).unsqueeze(0).expand(n, -1, -1, -1, -1)
    fm = fr[:, :, 0].contiguous().cuda()
    fa = fr[:, :, 1].contiguous().cuda() if mode == 1 else None
    enc.set_state_all(native.STATE_RNG_PY, np.stack(py_states))
    enc.set_state_all(native.STATE_RNG_NP, np.stack(np_states))
    return enc, fm, fa


def _device_run(native, device_tables, mode, frames, sched, py_states, np_states, kernel, **options):
    enc, fm, fa = _encoder(native, device_tables, mode, frames, py_states, np_states, kernel, **options)
    ops = enc.encode(fm, fa, sched)
    enc.check()
    return enc, ops.cpu().numpy()


def _state_of(native, enc, mode, i):
    return {"mem": [enc.get_state(native.STATE_MEM_MAIN + b, i) for b in range(mode + 1)],
            "up": [enc.get_state(native.STATE_UP_MAIN + b, i) for b in range(mode + 1)],
            "draws": tuple(int(x) for x in enc.get_state(native.STATE_COUNTERS, i)[:2]),
            "py": enc.get_state(native.STATE_RNG_PY, i), "np": enc.get_state(native.STATE_RNG_NP, i)}


def _same_stream(got, want, what):
    g, w = mt_model.canonical(got), mt_model.canonical(want)
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, "%s: canonical state differs in %d words, first at %d (624 = the index): got %d (raw index %d), want %d" % (
        what, len(bad), bad[0], g[bad[0]], got[624], w[bad[0]])


def _compare(native, enc, mode, ops, i, ref, tag):
    tag = "%s, stream %d" % (tag, i)
    bad = np.nonzero((ops[i] != ref["ops"]).any(axis=1))[0]
    assert len(bad) == 0, "%s: first opcode mismatch at %d: got %s want %s" % (tag, bad[0], ops[i][bad[0]], ref["ops"][bad[0]])
    st = _state_of(native, enc, mode, i)
    for b in range(mode + 1):
        assert np.array_equal(st["mem"][b], ref["mem"][b]), "%s: memory map of bank %d" % (tag, b)
        assert np.array_equal(st["up"][b], ref["up"][b]), "%s: priorities of bank %d" % (tag, b)
    assert st["draws"] == ref["draws"], "%s: draw counters %s, oracle %s" % (tag, st["draws"], ref["draws"])
    _same_stream(st["py"], ref["py"], tag + ", random")
    _same_stream(st["np"], ref["np"], tag + ", np.random")
    return st


def _iid_frame(mode, seed):
    """one frame the way test_gpu_encode._synth makes them"""
    from test_gpu_encode import _synth
    return _synth(mode, 1, seed)[0]


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
    _same_stream(got[624]["py"], got[625]["py"], tag + ", streams 624 and 625, random")
    _same_stream(got[624]["np"], got[625]["np"], tag + ", streams 624 and 625, np.random")
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
            back = _state_of(native, enc, mode, 0)
            assert np.array_equal(back["py"], py[0]) and np.array_equal(back["np"], npw[0]) and back["draws"] == (0, 0)
        ops = enc.encode(fm, fa, sched).cpu().numpy()
        enc.check()
        runs.append((ops, _compare(native, enc, mode, ops, 0, ref, "kernel %r, %s" % (kernel, "after the rollback" if again else "first run"))))
    assert np.array_equal(runs[0][0], runs[1][0])
    _same_stream(runs[1][1]["py"], runs[0][1]["py"], "random, second run against the first")
    _same_stream(runs[1][1]["np"], runs[0][1]["np"], "np.random, second run against the first")
    enc.close()
