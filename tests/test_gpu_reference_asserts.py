"""GPU: every kernel form held to the reference's asserts, step for step (inputs: tests/assert_inputs.py; what they do, on
the CPU: tests/test_assert_inputs_host.py).

Input the reference ACCEPTS although it is not tidy -- bytes in the target's screen holes, bit 7 on DHGR bytes that are never
popped or sort behind the budget -- gives the oracle's opcodes and state in every form (a); input it REFUSES stops the stream
at the oracle's step, with the oracle's opcodes in front, names the right stream, code and line, and leaves the streams beside
it alone (b-f, h).  Forms: the four greedy kernels ("team", one wave per stream in its plain and LDS-shared forms and as
dispatched, the workgroup kernel), the fourth offset, both joint content choices in their home kernel.

Out of reach, so without a test: video.py:124 (a popped hole: the prologue zeroes a hole's weight, :111, and a hole is never
an extra offset), video.py:154-155 (a primary's own delta cannot be negative once :141 has zeroed its weight; hole deltas
are never negative), video.py:137 on an entry popped from the RE-QUEUED bag (iiv_team.h's phase B, the bag branch of the other
kernels): a byte is re-queued only as an extra offset, which needs a priority != 0 (:159), which within a generator only a
byte with a priority != 0 at its start can have -- and that byte has an entry in the initial list, whose key is negative and
so pops in front of every re-queued one (their keys are 65536 - p > 0); popped there with its priority still != 0 it is the
primary and :137 fires THERE, with priority 0 it is dead for the rest of the generator.  So no bit-7 byte reaches the bag
alive.  And the encoder's internal limits (pushed-entry capacity, loop guard, sort budget, bank mix), which
valid use cannot reach.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import assert_inputs as A
import encode_harness as H

pytestmark = pytest.mark.gpu

GREEDY = ["team", True, "plain", "shared", False]
FOURTH = ["team", "shared", True]
FORMS = [(k, False) for k in GREEDY] + [(k, True) for k in FOURTH]          # (greedy kernel, fourth offset)
JOINT = [True, "split"]                                                       # both content choices; home: the workgroup kernel
JOINT_CAP = 40                                                                # (the oracle's joint step is slow)


class Batch:
    """an encoder over one clip per stream, every stream seeded as its oracle run is"""

    def __init__(self, native, O, device_tables, mode, clips, seeds, kernel=None, fourth=False, joint=False, dw=None):
        self.native, self.mode, self.n, self.kernel = native, mode, len(clips), kernel
        named = {k: v for k, v in (("kernel", kernel), ("dw", dw)) if v is not None}
        self.enc = H.make_encoder(native, device_tables, mode, 5, self.n, fourth=fourth, joint=joint, rng=list(seeds), O=O, **named)
        self.enc.profile(True)
        self.fm, self.fa = H.device_frames(mode, clips)

    def encode(self, scheds):
        ops, _ = self.enc.encode_streams(self.fm, self.fa, scheds)
        return ops.cpu().numpy()

    def check(self):
        """iiv_encoder_check -> (code, bad_stream or -1, message)"""
        bad = C.c_int(-1)
        rc = self.native.lib().iiv_encoder_check(self.enc._h, C.byref(bad), self.native.stream_ptr())
        return rc, bad.value, self.native.lib().iiv_last_error().decode("utf-8", "replace") if rc else ""

    def state(self, i):
        """stream i's state as the device holds it now (encode_harness.State)"""
        return H.device_state(self.native, self.enc, i, self.mode)

    def same_state(self, i, want, tag, fields=H.FIELDS):
        """stream i against an oracle's (or the stream's own earlier) State"""
        H.check_oracle_state(self.native, self.enc, i, want, self.mode, str(tag), fields)

    def close(self):
        """the kernel asked for is the one that ran, and no other (a silent fall-back must not pass), in every test"""
        forms = self.enc.launch_forms()
        if self.kernel is not None and sum(forms.values()):
            assert A.ran(self.kernel, forms), (self.kernel, forms)
        self.enc.close()


# a stream that an assert stopped: the reference raises out of the step, so only what the steps before it stored is defined
STOPPED = ("mem", "packed")


def _otab(oracle_tables, mode):
    return oracle_tables.get(mode, 5)


# ---- a. accepted input equals the oracle, in every form

def _accepted(O, table, mode, name, cap=None, fourth=False, joint=False):
    """(clip, schedule, seeds) of an input the reference accepts"""
    if name == "dirty_holes":
        return A.dirty_holes(mode), A.dirty_holes_schedule(mode, cap), A.SEEDS["dirty_holes"]
    if name == "quiet":
        frames, sched = A.quiet_palette_bit(O, table, mode, cap, fourth, joint)
        return frames, sched, A.SEEDS["quiet"]
    sched = [(f, a, r, min(k, cap) if cap else k) for (f, a, r, k) in A.late_short(fourth)]
    return A.late_palette_bit(mode), sched, A.SEEDS["late"]


@pytest.mark.parametrize("mode,name", [(A.DHGR, "dirty_holes"), (A.HGR, "dirty_holes"), (A.DHGR, "quiet"), (A.DHGR, "late_short")])
def test_accepted_inputs_equal_the_oracle_in_every_form(native, O, oracle_tables, device_tables, mode, name):
    """opcodes, both memory maps, priorities, packed screen, draw counters and both generators' states; check() clean"""
    table = _otab(oracle_tables, mode)
    ran = set()
    for fourth in (False, True):
        frames, sched, seeds = _accepted(O, table, mode, name, fourth=fourth)
        v, want, code = A.oracle_run(O, mode, table, frames, sched, seeds, fourth=fourth)
        assert code == 0
        wstate = H.oracle_state(v, mode)
        for kernel, f in FORMS:
            if f != fourth:
                continue
            b = Batch(native, O, device_tables, mode, [frames], [seeds], kernel, fourth)
            ops = b.encode([sched])
            assert b.check() == (0, -1, ""), (kernel, fourth)
            forms = b.enc.launch_forms()
            assert A.ran(kernel, forms), (kernel, fourth, forms)
            ran |= {k for k, n in forms.items() if n}
            H.check_ops(ops[0], want, (name, mode, kernel, fourth))
            b.same_state(0, wstate, (name, mode, kernel, fourth))
            b.close()
        framesj, schedj, seeds = _accepted(O, table, mode, name, cap=JOINT_CAP, fourth=fourth, joint=True)
        vj, wantj, code = A.oracle_run(O, mode, table, framesj, schedj, seeds, fourth=fourth, joint=True)
        assert code == 0
        for joint in JOINT:
            b = Batch(native, O, device_tables, mode, [framesj], [seeds], None, fourth, joint)
            ops = b.encode([schedj])
            assert b.check() == (0, -1, ""), (joint, fourth)
            assert A.ran(False, b.enc.launch_forms()), (joint, fourth, b.enc.launch_forms())
            H.check_ops(ops[0], wantj, (name, mode, "joint", joint, fourth))
            b.same_state(0, H.oracle_state(vj, mode), (name, mode, "joint", joint, fourth))
            b.close()
    assert ran == {"plain", "shared", "team", "workgroup"}


# ---- b, c. the assert fires where the reference's fires; an errored stream stays out

_four = {}


def _four_streams(O, oracle_tables, fourth):
    """streams 0 and 3 clean, 1 = early_palette_bit, 2 = late_palette_bit; two calls; every stream's oracle run (cached)"""
    if fourth in _four:
        return _four[fourth]
    table = _otab(oracle_tables, A.DHGR)
    first, second = A.clean_schedules(A.DHGR)
    clips = [A.clean(A.DHGR, "clean"), A.early_palette_bit(), A.late_palette_bit(), A.clean(A.DHGR, "clean2")]
    seeds = [A.SEEDS["clean"], A.SEEDS["early"], A.SEEDS["late"], A.SEEDS["clean2"]]
    calls = [[first, A.EARLY_SCHEDULE_BEHIND_AUX, A.late_short(fourth), first], [second, [(0, 0, 0, 20)], A.LATE_MORE, second]]
    runs = []
    for i in range(4):
        v, ops1, code1 = A.oracle_run(O, A.DHGR, table, clips[i], calls[0][i], seeds[i], fourth=fourth)
        st1 = H.oracle_state(v, A.DHGR)
        ops2, code2, st2 = None, code1, st1
        if not code1:
            _, ops2, code2 = A.oracle_run(O, A.DHGR, table, clips[i], calls[1][i], seeds[i], fourth=fourth, v=v)
            st2 = H.oracle_state(v, A.DHGR)
        runs.append(dict(ops=[ops1, ops2], code=[code1, code2], state=[st1, st2]))
    assert [r["code"] for r in runs] == [[0, 0], [A.ERR_PALETTE_BIT] * 2, [0, A.ERR_PALETTE_BIT], [0, 0]]
    assert 30 < len(runs[1]["ops"][0]) < 230 and 0 < len(runs[2]["ops"][1]) < A.LATE_MORE[0][3]
    _four[fourth] = (clips, seeds, calls, runs)
    return _four[fourth]


def _names_stream(native, got, stream, line):
    rc, bad, msg = got
    assert rc == native.ERR_ASSERT and bad == stream, got
    assert ("stream %d:" % stream) in msg and line in msg, msg


@pytest.mark.parametrize("kernel,fourth", FORMS)
def test_the_assert_fires_where_the_references_fires(native, O, oracle_tables, device_tables, kernel, fourth):
    clips, seeds, calls, runs = _four_streams(O, oracle_tables, fourth)
    b = Batch(native, O, device_tables, A.DHGR, clips, seeds, kernel, fourth)
    tag = (kernel, fourth)
    # -- the first call: stream 1 stops at the oracle's step, stream 2's byte is still behind the budget
    ops = b.encode(calls[0])
    _names_stream(native, b.check(), 1, A.MSG_137)
    assert A.ran(kernel, b.enc.launch_forms()), (tag, b.enc.launch_forms())
    n_ok = len(runs[1]["ops"][0])
    H.check_ops(ops[1][:n_ok], runs[1]["ops"][0], (tag, "stream 1, the opcodes in front of the assert"))
    b.same_state(1, runs[1]["state"][0], (tag, "stream 1 stopped there"), STOPPED)
    for i in (0, 2, 3):
        want = runs[i]["ops"][0]
        H.check_ops(ops[i][:len(want)], want, (tag, "call 1, stream", i))
        b.same_state(i, runs[i]["state"][0], (tag, "call 1, stream", i))
    # -- c: stream 1 stays out of the next call (which asks it to go on), whatever the others do
    before = b.state(1)
    ops = b.encode(calls[1])
    _names_stream(native, b.check(), 1, A.MSG_137)
    b.same_state(1, before, (tag, "stream 1 after a further call"))
    # -- the continuation: stream 2 stops at the oracle's index; 0 and 3 are exact across both calls
    n_ok2 = len(runs[2]["ops"][1])
    assert n_ok2 == A.LATE_MORE_INDEX
    H.check_ops(ops[2][:n_ok2], runs[2]["ops"][1], (tag, "stream 2, the opcodes in front of the assert"))
    b.same_state(2, runs[2]["state"][1], (tag, "stream 2 stopped there"), STOPPED)
    for i in (0, 3):
        want = runs[i]["ops"][1]
        H.check_ops(ops[i][:len(want)], want, (tag, "call 2, stream", i))
        b.same_state(i, runs[i]["state"][1], (tag, "call 2, stream", i))
    # -- and a call that STARTS generators: streams 1 and 2 stay as they are (no prologue runs on them), check() still says 1
    before = [b.state(i) for i in (1, 2)]
    b.encode([[(2, 1, 1, 30)]] * 4)
    _names_stream(native, b.check(), 1, A.MSG_137)
    for k, i in enumerate((1, 2)):
        b.same_state(i, before[k], (tag, "stream %d after a further restart" % i))
    b.close()


@pytest.mark.parametrize("kernel", GREEDY)
def test_rollback_clears_the_error_and_the_opcodes_in_front_of_it_are_the_oracles(native, O, oracle_tables, device_tables, kernel):
    """what clears a stream's error is the state coming back: a snapshot from before the bad launch, rolled back"""
    clips, seeds, calls, runs = _four_streams(O, oracle_tables, False)
    b = Batch(native, O, device_tables, A.DHGR, clips[:2], seeds[:2], kernel)
    n_ok = len(runs[1]["ops"][0])
    b.enc.snapshot()
    b.encode([calls[0][0], calls[0][1]])
    _names_stream(native, b.check(), 1, A.MSG_137)
    b.enc.rollback()
    assert b.check() == (0, -1, "")
    ops = b.encode([calls[0][0], [calls[0][1][0], (0, 0, 1, n_ok - 30)]])
    assert b.check() == (0, -1, "")
    H.check_ops(ops[1][:n_ok], runs[1]["ops"][0], (kernel, "the n_ok opcodes"))
    b.same_state(1, runs[1]["state"][0], (kernel, "the state in front of the assert"))
    H.check_ops(ops[0], runs[0]["ops"][0], (kernel, "stream 0"))
    # one more opcode is the one that asserts
    b.encode([[], [(0, 0, 0, 1)]])
    _names_stream(native, b.check(), 1, A.MSG_137)
    b.close()


# ---- d. the lowest stream wins, with its own message

def _hole_map(bank_value=0x11):
    m = np.zeros((32, 256), np.uint8)
    m[7, 123] = bank_value
    return m


@pytest.mark.parametrize("kernel", ["team", True, False])
def test_the_lowest_bad_stream_is_reported_with_its_own_message(native, O, oracle_tables, device_tables, kernel):
    clips = [A.clean(A.DHGR)] * 8
    clips[5] = A.early_palette_bit()
    b = Batch(native, O, device_tables, A.DHGR, clips, [A.SEEDS["early"]] * 8, kernel)
    b.enc.set_state(native.STATE_MEM_MAIN, _hole_map(), 2)
    b.encode([A.EARLY_SCHEDULE] * 8)
    _names_stream(native, b.check(), 2, A.MSG_87)
    b.close()
    # the other way round: the palette bit in the lower stream
    clips = [A.clean(A.DHGR)] * 8
    clips[2] = A.early_palette_bit()
    b = Batch(native, O, device_tables, A.DHGR, clips, [A.SEEDS["early"]] * 8, kernel)
    b.enc.set_state(native.STATE_MEM_MAIN, _hole_map(), 5)
    b.encode([A.EARLY_SCHEDULE] * 8)
    _names_stream(native, b.check(), 2, A.MSG_137)
    b.close()


# ---- e. video.py:87

@pytest.mark.parametrize("mode,bank", [(A.DHGR, 0), (A.DHGR, 1), (A.HGR, 0)])
def test_a_byte_in_the_memory_maps_hole_stops_the_generator_before_it_draws(native, O, oracle_tables, device_tables, mode, bank):
    """the prologue reports :87 in front of np.random's draw, as the reference raises in front of it: the stream's draw counters
    and both generators stay where they were; the neighbouring streams are exact; the other bank's hole does not fire"""
    table = _otab(oracle_tables, mode)
    clip, seeds = A.clean(mode), A.SEEDS["clean"]
    sched = [(0, bank, 1, 60)]
    drawn = []
    for kernel in ("team", True, False):
        b = Batch(native, O, device_tables, mode, [clip] * 3, [seeds] * 3, kernel)
        b.enc.set_state(native.STATE_MEM_MAIN + bank, _hole_map(), 1)
        before = b.state(1)
        ops = b.encode([sched] * 3)
        _names_stream(native, b.check(), 1, A.MSG_87)
        drawn.append((kernel, before, b.state(1)))
        v, want, code = A.oracle_run(O, mode, table, clip, sched, seeds)
        for i in (0, 2):
            H.check_ops(ops[i], want, (kernel, "neighbour", i))
            b.same_state(i, H.oracle_state(v, mode), (kernel, "neighbour", i))
        b.close()
    # the oracle agrees: code -1, nothing drawn
    v = A.oracle_video(O, mode, table, seeds)
    v.memory(bank)[7, 123] = 0x11
    _, got, code = A.oracle_run(O, mode, table, clip, sched, seeds, v=v)
    assert code == A.ERR_HOLES and len(got) == 0 and v.draws() == (0, 0)
    if mode == A.DHGR:
        # a hole byte in the OTHER bank's map does not fire: the reference looks at the generator's own bank
        v = A.oracle_video(O, mode, table, seeds)
        v.memory(1 - bank)[7, 123] = 0x11
        v.packed[:] = O.pack(mode, v.memory(0), v.memory(1))          # (a map loaded with that byte is packed with it)
        _, want, code = A.oracle_run(O, mode, table, clip, sched, seeds, v=v)
        assert code == 0
        for kernel in ("team", True, False):
            b = Batch(native, O, device_tables, mode, [clip], [seeds], kernel)
            b.enc.set_state(native.STATE_MEM_MAIN + 1 - bank, _hole_map())
            ops = b.encode([sched])
            assert b.check() == (0, -1, ""), kernel
            H.check_ops(ops[0], want, (kernel, "other bank's hole"))
            b.same_state(0, H.oracle_state(v, mode), (kernel, "other bank's hole"))
            b.close()
    # the reference raises in front of its draw (oracle: gen_prologue returns before draw_np): nothing is drawn
    for kernel, before, after in drawn:
        assert after.draws == before.draws == (0, 0), (kernel, after.draws)
        assert np.array_equal(after.py, before.py) and np.array_equal(after.np, before.np), kernel


# ---- f. video.py:117

def _plant_sites(clip, mode):
    """(a byte that differs from the target on a black screen and has a diff weight, a byte that equals it with all its
    window: its priority is zeroed by :115)"""
    tgt = clip[0, 0]
    differs = (9, int(np.nonzero(tgt[9, :100])[0][3]))
    quiet = np.zeros((32, 256), bool)
    z = tgt == 0
    if mode == A.DHGR:
        z &= clip[0, 1] == 0
    quiet[:, 1:-1] = z[:, 1:-1] & z[:, :-2] & z[:, 2:]
    quiet[:, A.HOLES] = False
    p, o = np.argwhere(quiet)[0] if quiet.any() else (None, None)
    return differs, (int(p), int(o))


@pytest.mark.parametrize("mode", A.MODES)
def test_negative_priorities(native, O, oracle_tables, device_tables, mode):
    """a planted negative priority fires :117 where the byte has a diff weight, and is zeroed by :115 where it has none;
    -1, -65535 and -70000 -- both sides of the 16-bit copy's hand-over -- never come back as large positive priorities"""
    table = _otab(oracle_tables, mode)
    clip = A.clean(mode).copy()
    clip[0, :, 20:24, 30:60] = 0                                  # (a black patch: bytes that equal the black screen)
    seeds = A.SEEDS["clean"]
    sched = [(0, 0, 1, 120), (1, 0, 1, 60)]
    differs, equal = _plant_sites(clip, mode)
    v, clean_ops, code = A.oracle_run(O, mode, table, clip, sched, seeds)
    assert code == 0
    for kernel in ("team", True, False):
        for value in (-5000, -1, -65535, -70000):
            # the byte that differs: dw - |value| < 0 for all of these but -1, where the oracle decides
            up = np.zeros((32, 256), np.int32)
            up[differs] = value
            vo = A.oracle_video(O, mode, table, seeds)
            vo.update_priority(0)[differs] = value
            _, want, wcode = A.oracle_run(O, mode, table, clip, sched, seeds, v=vo)
            assert wcode == (0 if value == -1 else A.ERR_NEGATIVE), (value, wcode)
            b = Batch(native, O, device_tables, mode, [clip] * 2, [seeds] * 2, kernel)
            b.enc.set_state(native.STATE_UP_MAIN, up, 1)
            assert np.array_equal(b.enc.get_state(native.STATE_UP_MAIN, 1), up)        # through the 16-bit copy and back
            ops = b.encode([sched] * 2)
            if wcode:
                _names_stream(native, b.check(), 1, A.MSG_117)
                assert b.state(1).draws == (0, 0), (kernel, value)          # (raised in front of the draw)
            else:
                assert b.check() == (0, -1, ""), (kernel, value)
                H.check_ops(ops[1], want, (kernel, value, "planted stream"))
                b.same_state(1, H.oracle_state(vo, mode), (kernel, value, "planted stream"))
            H.check_ops(ops[0], clean_ops, (kernel, value, "neighbour"))
            b.close()
            # the byte that equals the target: zeroed by :115, never fires, the opcodes are a clean stream's
            up = np.zeros((32, 256), np.int32)
            up[equal] = value
            b = Batch(native, O, device_tables, mode, [clip], [seeds], kernel)
            b.enc.set_state(native.STATE_UP_MAIN, up)
            ops = b.encode([sched])
            assert b.check() == (0, -1, ""), (kernel, value)
            H.check_ops(ops[0], clean_ops, (kernel, value, "zeroed plant"))
            b.same_state(0, H.oracle_state(v, mode), (kernel, value, "zeroed plant"))
            b.close()


# ---- g. no generator

def test_a_continuation_without_a_generator_is_refused(native, O, device_tables):
    clip = A.clean(A.DHGR)
    b = Batch(native, O, device_tables, A.DHGR, [clip], [A.SEEDS["clean"]])
    with pytest.raises(native.IIVError) as e:
        b.enc.encode(b.fm, b.fa, [(0, 0, 0, 5)])
    assert e.value.code == native.ERR_INVALID and "continues no generator" in str(e.value)
    with pytest.raises(native.IIVError) as e:
        b.enc.encode_streams(b.fm, b.fa, [[(0, 0, 0, 5)]])
    assert e.value.code == native.ERR_INVALID and "continues no generator" in str(e.value)
    assert b.check() == (0, -1, "")                                  # (refused on the host: nothing was launched)
    b.close()


# ---- h. persistent workgroups: errored streams among thousands

def test_errored_streams_in_the_persistent_workgroups_queue(native, O, oracle_tables, device_tables):
    """4608 + 5 streams (test_gpu_properties.test_kernel_forms_agree_at_batch_sizes: the LDS-shared form's 512 resident
    workgroups of eight streams take more than one round off their queue, the last workgroup partly filled), tiled from eight
    clips, one generator of 60 opcodes; every 97th stream from 40 on is early_palette_bit under one of twelve seed pairs with
    which the reference asserts 13 to 50 opcodes into the generator: streams that emit for a while and then stop, among
    streams that go on."""
    import torch
    S, K = 4608 + 5, 60
    table = _otab(oracle_tables, A.DHGR)
    base = [A.picture(A.DHGR, 900 + i, 1) for i in range(8)]
    bad_clip = A.early_palette_bit()[:1]
    bad = list(range(40, S, 97))
    seeds = [(i + 1, 2 * i + 3) for i in range(S)]
    bad_seeds = [(a, 2 * a + 1) for a in (2, 4, 5, 10, 15, 16, 22, 25, 35, 36, 44, 46)]
    bad_ops = []
    for sd in bad_seeds:
        _, got, code = A.oracle_run(O, A.DHGR, table, bad_clip, [(0, 0, 1, K)], sd)
        assert code == A.ERR_PALETTE_BIT and 10 <= len(got) <= 50, (sd, code, len(got))
        bad_ops.append(got)
    for k, i in enumerate(bad):
        seeds[i] = bad_seeds[k % len(bad_seeds)]
    fr = np.stack([base[i % 8][0] for i in range(S)])
    fr[bad] = bad_clip[0]
    fm = torch.from_numpy(np.ascontiguousarray(fr[:, None, 0])).cuda()
    fa = torch.from_numpy(np.ascontiguousarray(fr[:, None, 1])).cuda()
    res = {}
    for kernel in ("plain", "shared"):
        enc = H.make_encoder(native, device_tables, A.DHGR, 5, S, kernel=kernel, rng=seeds, O=O)
        enc.profile(True)
        ops = enc.encode(fm, fa, [(0, 0, 1, K)])
        bad_stream = C.c_int(-1)
        rc = native.lib().iiv_encoder_check(enc._h, C.byref(bad_stream), native.stream_ptr())
        msg = native.lib().iiv_last_error().decode()
        assert rc == native.ERR_ASSERT and bad_stream.value == bad[0] and ("stream %d:" % bad[0]) in msg and A.MSG_137 in msg, (rc, msg)
        assert A.ran(kernel, enc.launch_forms()), (kernel, enc.launch_forms())
        res[kernel] = ops
        enc.close()
    good = torch.ones(S, dtype=torch.bool, device="cuda")
    good[bad] = False
    assert torch.equal(res["plain"][good], res["shared"][good])              # every clean stream, on the device
    for kernel in ("plain", "shared"):                                       # the bad ones: the oracle's opcodes in front of the assert
        got = res[kernel][bad[:24]].cpu().numpy()
        for k in range(24):
            want = bad_ops[k % len(bad_seeds)]
            H.check_ops(got[k][:len(want)], want, (kernel, "bad stream", bad[k]))
    sample = sorted({0, S - 1} | {i + 1 for i in bad[:14]})
    assert len(sample) == 16
    shared = res["shared"][sample].cpu().numpy()
    for j, i in enumerate(sample):
        _, want, code = A.oracle_run(O, A.DHGR, table, fr[i][None], [(0, 0, 1, K)], seeds[i])
        assert code == 0
        H.check_ops(shared[j], want, ("stream", i))
