"""GPU: the library's first-use and grow-on-demand paths taken while earlier work of the same object is still queued on a
sleeping, non-blocking side stream.  tests/test_gpu_stream_order.py warms every path up before its probe, on
purpose; here nothing is warmed up: a buffer allocated, uploaded or re-allocated inside the call under test is ordered against
the work in flight by hand-written waits only, and on the null stream, which orders itself against everything, a misplaced one
gives the right bytes.  The probe is tests/stream_probe.py's, the yardsticks the oracle, resize_model and yuv_model, the
comparisons `==` on bytes.  Where the code under test waits on the host by design the `busy` condition is dropped, and the
docstring names the line.  One wait is kept out of the way on purpose: a fresh encoder holds no descriptor buffer, so its first
encode grows from nothing and waits for its stream (csrc/iiv_encode.hip upload_segs, d_segs.count() == 0); every encoder case
makes that first encode -- Calls.prime, on the idle null stream, the oracle making it too -- BEFORE the sleep, so that the
sequence under test is enqueued while the stream really sleeps.  The constants and sequences are tests/cold_cases.py's; tests/test_cold_paths_host.py holds them to
csrc/ and shows on the CPU that every sequence crosses the boundary it is named after."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import cold_cases as CC
import cold_shared_child
import encode_harness as H
import resize_model
import yuv_model
from device_guards import ok
from stream_cases import Enc, dp as _dp, frames as _frames
from stream_probe import Probe, SLEEP_CYCLES

pytestmark = pytest.mark.gpu

HGR, DHGR = 0, 1
MODES = [DHGR, HGR]


def _np(t):
    return t.cpu().numpy()


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


class Calls:
    """One encoder on one probe: its frames over decoys, and the calls of a sequence as steps -- step(stream pointer) makes one
    call and scribbles over that call's host arrays at once."""

    def __init__(self, native, e, seed, probe=None):
        self.native, self.e, self.mode, self.n = native, e, e.mode, e.n
        self.p = probe or Probe()
        self.fm, self.fa = _frames(self.mode, self.n, 2, seed)
        self.dm, self.da = _frames(self.mode, self.n, 2, seed + 1)
        self.d_main, self.d_aux = self.p.input(self.fm, self.dm), self.p.input(self.fa, self.da)
        self.prime()

    def prime(self, n_segments=CC.PRIME_SEGMENTS):
        """The encoder's first encode, on the idle null stream and synchronised, of the decoy frames the device holds now:
        d_segs, pinned slot 0 and (under a one-wave form) d_queue go from nothing to twice n_segments here, not behind the sleep."""
        import torch
        native = self.native
        segments = [(j % 2, 0, 1, 12 + j) for j in range(n_segments)]
        ops = torch.zeros((self.n, sum(s[3] for s in segments), 6), dtype=torch.uint8, device="cuda")
        ok(native, native.lib().iiv_encode(self.e.enc._h, _dp(self.d_main), self._aux(), 2, native.segment_array(segments), n_segments,
                                           _dp(ops), native.stream_ptr()))
        self.e.enc.check()
        torch.cuda.synchronize()
        got = _np(ops)
        for i in range(self.n):
            H.check_ops(got[i], self.e.oracle(i, self.dm, self.da, segments), "priming call, stream %d" % i)

    def _aux(self):
        return _dp(self.d_aux if self.mode == DHGR else None)

    def encode(self, segments):
        """-> (step, the call's output, filled with the sentinels by the probe)"""
        native, L = self.native, self.native.lib()
        ops = self.p.output((self.n, sum(s[3] for s in segments), 6))
        segs = native.segment_array(segments)

        def step(st):
            ok(native, L.iiv_encode(self.e.enc._h, _dp(self.d_main), self._aux(), 2, segs, len(segments), _dp(ops), st))
            for j, (f, a, r, k) in enumerate(segments):          # another frame, in range, no more opcodes
                segs[j].frame, segs[j].is_aux, segs[j].restart, segs[j].n_ops = 1 - f, 0, 1, max(k // 2, 1)
        return step, ops

    def want(self, i, segments):
        """stream i's oracle run on through `segments`"""
        return self.e.oracle(i, self.fm, self.fa, segments)

    def check_state(self, tag):
        for i, v in enumerate(self.e.videos):
            H.check_oracle_state(self.native, self.e.enc, i, v, self.mode, "%s, stream %d" % (tag, i))


def _run(p, steps, asynchronous):
    p.run(lambda st: [s(st) for s in steps], asynchronous=asynchronous)


# ---- cases 1 and 2: the launch descriptors and the stream counters grow ----------------------------------------------------

def _grow_sequence(calls):
    """encodes A, B, C of CC.GROW_SEGMENTS -> (steps, check)"""
    plan = [CC.grow_segments(calls.mode, n, j) for j, n in enumerate(CC.GROW_SEGMENTS)]
    made = [calls.encode(s) for s in plan]

    def check(tag):
        calls.e.enc.check()
        for name, segments, (_, ops) in zip("ABC", plan, made):
            got = _np(ops)
            for i in range(calls.n):
                H.check_ops(got[i], calls.want(i, segments), "%s: call %s, stream %d" % (tag, name, i))
        calls.check_state(tag)
    return [s for s, _ in made], check


@pytest.mark.parametrize("mode", MODES)
def test_descriptors_grow_behind_a_live_call(native, O, device_tables, oracle_tables, mode):
    """Case 1.  Behind the priming call (d_segs 2, pinned slot 0 of 2): A (1 descriptor, the unused slot 1) is enqueued behind
    the sleep and waits for nothing; B (3) exceeds d_segs' 2 and re-allocates it with A still asleep, C (7) exceeds the 6 again
    and finds the pinned slot A used, 2 entries, too small (csrc/iiv_encode.hip upload_segs: d_segs.alloc behind
    hipStreamSynchronize(st), h_segs[k].alloc behind the slot's hipEventSynchronize).  B's wait is on the host: no `busy`."""
    e = Enc(native, O, device_tables, oracle_tables, mode, 2, 111)
    calls = Calls(native, e, 1400 + mode)
    steps, check = _grow_sequence(calls)
    _run(calls.p, steps, asynchronous=False)
    check("descriptor grow")
    e.close()


@pytest.mark.parametrize("kernel", ["plain", "shared"])
@pytest.mark.parametrize("mode", MODES)
def test_stream_counters_grow_behind_a_live_call(native, O, device_tables, oracle_tables, mode, kernel):
    """Case 2.  The same sequence under a forced one-wave form (LaunchChoice::zeroed_queue): the priming call leaves 2 counters,
    A's one round fits and sleeps, B's 3 launch rounds exceed the 2, C's 7 the 6 after B (reset_queues: d_queue.alloc behind hipStreamSynchronize(st), then the
    memset on st).  The wait is on the host: no `busy`."""
    e = Enc(native, O, device_tables, oracle_tables, mode, 2, 121, kernel=kernel)
    calls = Calls(native, e, 1410 + mode)
    steps, check = _grow_sequence(calls)
    e.enc.profile(True)
    _run(calls.p, steps, asynchronous=False)
    check("counter grow, " + kernel)
    ran = e.enc.launch_forms()
    assert ran[kernel] == sum(CC.GROW_SEGMENTS) == sum(ran.values()), ran      # (profiling starts behind the priming call)
    e.close()


# ---- case 3: the small-state staging ring, first use and wrap --------------------------------------------------------------

def _ring_sequence(calls, O, seed, stream_1=()):
    """encode, CC.RING_CALLS iiv_encoder_set_state_async calls of different valid contents, encode -> (steps, check)"""
    native, L, e = calls.native, calls.native.lib(), calls.e
    b = 1 if calls.mode == DHGR else 0
    seg_a, seg_b = [(0, 0, 1, 30), (0, 0, 0, 25)], [(1, b, 1, 35), (1, b, 0, 20)]
    (step_a, ops_a), (step_b, ops_b) = calls.encode(seg_a), calls.encode(seg_b)
    what_of = {"RNG_PY": native.STATE_RNG_PY, "RNG_NP": native.STATE_RNG_NP, "OUT_OF_WORK": native.STATE_OUT_OF_WORK}
    plan = CC.ring_plan(stream_1)
    last = {(kind, s): i for i, (kind, s) in enumerate(plan)}       # the call whose contents the second encode starts from
    steps, set_last = [step_a], {}
    for i, (kind, s) in enumerate(plan):
        if kind == "OUT_OF_WORK":       # (the oracle can only clear the flags: the last set clears them, the others raise them)
            value = np.array([0, 0] if last[(kind, s)] == i else [1, 1], np.int32)
            other = 1 - value
        else:
            py, npw = H.seed_states(O, seed + 2 * i, seed + 2 * i + 1)
            py2, np2 = H.seed_states(O, seed + 500 + i, seed + 600 + i)
            value, other = (py, py2) if kind == "RNG_PY" else (npw, np2)
        if last[(kind, s)] == i:
            set_last[(kind, s)] = value.copy()
        buf = np.ascontiguousarray(value).copy()

        def step(st, buf=buf, other=other, what=what_of[kind], s=s):
            ok(native, L.iiv_encoder_set_state_async(e.enc._h, s, what, _hp(buf), buf.nbytes, st))
            buf[...] = other
        steps.append(step)
    steps.append(step_b)

    def check(tag):
        e.enc.check()
        got_a, got_b = _np(ops_a), _np(ops_b)
        for i in range(calls.n):
            H.check_ops(got_a[i], calls.want(i, seg_a), "%s: first encode, stream %d" % (tag, i))
        for (kind, s), value in set_last.items():
            v = e.videos[s]
            if kind == "RNG_PY":
                v.rng_py().set_state_words(value)
            elif kind == "RNG_NP":
                v.rng_np().set_state_words(value)
            else:
                assert not value.any()
                v.reset_out_of_work()
        for i in range(calls.n):
            H.check_ops(got_b[i], calls.want(i, seg_b), "%s: second encode, stream %d" % (tag, i))
        calls.check_state(tag)
    return steps, check


@pytest.mark.parametrize("stream_1", [(), CC.RING_STREAM_1], ids=["stream-0", "stream-1-in-between"])
@pytest.mark.parametrize("mode", MODES)
def test_small_ring_first_use_and_wrap(native, O, device_tables, oracle_tables, mode, stream_1):
    """Case 3.  The ring and its events are made by the first call, behind the sleeping encode; the fifth takes slot 0 again and
    waits for that slot's event (csrc/iiv_encoder.hip encoder_set_state_async: hipEventSynchronize(e->small_ev[k])) -- on the
    host, for the sleep to end: no `busy`.  The second encode starts from the last RNG_PY, RNG_NP and OUT_OF_WORK set.  With
    every call on stream 0 each first-round write is set again later, so that case holds the ring's advance and the final state
    only; in the variant stream 1's three items are set once each, two of them from slots that calls 5 and 6 take again for
    another item while the writes still sleep: without the wait they deliver the later calls' bytes."""
    e = Enc(native, O, device_tables, oracle_tables, mode, 2, 131)
    calls = Calls(native, e, 1420 + mode)
    steps, check = _ring_sequence(calls, O, 7000, stream_1)
    _run(calls.p, steps, asynchronous=False)
    check("small ring")
    e.close()


# ---- case 4: both snapshot slots first used behind an encode ---------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_snapshot_slots_first_used_behind_an_encode(native, O, device_tables, oracle_tables, mode):
    """Case 4.  A, snapshot_slot(1), B, snapshot_slot(0), C, rollback_slot(1), B', rollback_slot(0), C': each slot is allocated
    by its first snapshot (csrc/iiv_encoder.hip encoder_snapshot: a hipMalloc inside an enqueued call), both behind the sleep:
    A, the first snapshot, B and the second snapshot wait for nothing.  C takes A's pinned descriptor slot and waits on the host
    for A's copy, that is for the sleep (upload_segs' hipEventSynchronize): no `busy`."""
    L = native.lib()
    b = 1 if mode == DHGR else 0
    seg = {"A": [(0, 0, 1, 40)], "B": [(1, b, 1, 30), (1, b, 0, 20)], "C": [(0, b, 1, 25), (0, b, 0, 30)]}
    e = Enc(native, O, device_tables, oracle_tables, mode, 2, 141)
    calls = Calls(native, e, 1430 + mode)
    enc = {k: calls.encode(seg[k[0]]) for k in ("A", "B", "C", "B'", "C'")}

    def snapshot(slot):
        return lambda st: ok(native, L.iiv_encoder_snapshot_slot(e.enc._h, slot, st))

    def rollback(slot):
        return lambda st: ok(native, L.iiv_encoder_rollback_slot(e.enc._h, slot, st))
    _run(calls.p, [enc["A"][0], snapshot(1), enc["B"][0], snapshot(0), enc["C"][0], rollback(1), enc["B'"][0], rollback(0), enc["C'"][0]],
         asynchronous=False)
    e.enc.check()
    for i in range(2):
        for k in "ABC":
            want = calls.want(i, seg[k])
            H.check_ops(_np(enc[k][1])[i], want, "call %s, stream %d" % (k, i))
            if k != "A":
                H.check_ops(_np(enc[k + "'"][1])[i], want, "call %s', stream %d" % (k, i))
    calls.check_state("snapshot slots")
    e.close()


# ---- case 5: the live queues' first use ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_live_queues_first_used_on_the_side_stream(native, O, device_tables, oracle_tables, mode):
    """Case 5.  A one-stream encoder's first live calls: iiv_encoder_live_queue(0) (csrc/iiv_encode.hip encoder_live_queue: a
    coherent hipHostMalloc) and iiv_encode_live into it, then queue 1 and a call into it, all enqueued behind the sleep.  (Not
    the encoder's first call ever: that one waits for its stream, whatever it is -- the priming call is a plain iiv_encode.)
    Behind it nothing has to wait -- pinned slot 1 is unused, slot 0's copy long done: `busy` holds, against the sleep."""
    L = native.lib()
    b = 1 if mode == DHGR else 0
    segs = [(0, 0, 1, 60), (1, b, 1, 45)]
    tags = [0x1234, 0xFEDC]
    e = Enc(native, O, device_tables, oracle_tables, mode, 1, 151)
    calls = Calls(native, e, 1440 + mode)
    outs = [calls.p.output((1, s[3], 6)) for s in segs]
    arrs = [native.segment_array([s]) for s in segs]
    queues = []

    def call(st):
        for slot in (0, 1):
            addr, cap = C.c_void_p(0), C.c_int(0)
            ok(native, L.iiv_encoder_live_queue(e.enc._h, slot, C.byref(addr), C.byref(cap)))
            queues.append(np.frombuffer((C.c_uint64 * cap.value).from_address(addr.value), dtype=np.uint64))
            ok(native, L.iiv_encode_live(e.enc._h, _dp(calls.d_main), calls._aux(), 2, arrs[slot], 1, _dp(outs[slot]), slot, tags[slot], st))
            arrs[slot][0].frame, arrs[slot][0].n_ops = 1 - segs[slot][0], segs[slot][3] // 2
    calls.p.run(call)
    e.enc.check()
    for slot in (0, 1):
        want = calls.want(0, [segs[slot]])
        k = len(want)
        H.check_ops(_np(outs[slot])[0], want, "live call %d" % slot)
        rows = np.zeros((k, 8), np.uint8)
        rows[:, :6], rows[:, 6], rows[:, 7] = want, tags[slot] & 255, tags[slot] >> 8
        assert np.array_equal(queues[slot][:k], rows.view("<u8")[:, 0]), "queue %d" % slot
        assert not queues[slot][k:].any(), "queue %d: a slot behind the last opcode was written" % slot
    calls.check_state("live queues")
    e.close()


# ---- case 6: the tables iiv_encoder_set_option builds on first use ----------------------------------------------------------

OPTIONS = {"dw-split": ("OPT_DIFF_WEIGHTS", "DW_SPLIT", False), "joint-split": ("OPT_CONTENT_CHOICE", "CONTENT_JOINT_SPLIT", True),
           "joint": ("OPT_CONTENT_CHOICE", "CONTENT_JOINT", True)}


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("mode", MODES)
def test_set_option_builds_its_tables_behind_an_encode(native, O, device_tables, oracle_tables, mode, option):
    """Case 6.  A (default options, behind the priming call) sleeps on the side stream; iiv_encoder_set_option builds the split diff-weight, transposed or
    joint tables for the first time, on the default stream, and synchronises the device by contract (csrc/iiv_encoder.hip
    encoder_set_option: hipDeviceSynchronize behind each build) -- so no `busy`; B follows on the side stream at once, with no
    synchronise of the test's in between, and reads tables that must be complete."""
    L = native.lib()
    opt, value, joint = OPTIONS[option]
    b = 1 if mode == DHGR else 0
    seg_a, seg_b = [(0, 0, 1, 40), (0, 0, 0, 20)], [(1, b, 1, 45), (1, b, 0, 25)]
    e = Enc(native, O, device_tables, oracle_tables, mode, 2, 161)
    calls = Calls(native, e, 1450 + mode)
    (step_a, ops_a), (step_b, ops_b) = calls.encode(seg_a), calls.encode(seg_b)

    def set_option(st):
        ok(native, L.iiv_encoder_set_option(e.enc._h, getattr(native, opt), getattr(native, value)))
    _run(calls.p, [step_a, set_option, step_b], asynchronous=False)
    e.enc.check()
    for i in range(2):
        H.check_ops(_np(ops_a)[i], calls.want(i, seg_a), "%s: call A, stream %d" % (option, i))
    for v in e.videos:
        v.set_joint(joint)
    for i in range(2):
        H.check_ops(_np(ops_b)[i], calls.want(i, seg_b), "%s: call B, stream %d" % (option, i))
    calls.check_state(option)
    e.close()


# ---- case 7: cold resize tables ------------------------------------------------------------------------------------------

def _cold_resize(native, entry, h, w, H, W):
    """-> (got on the cold side-stream call, got on the warm second call, the model's)"""
    import torch
    L = native.lib()
    n = 2
    rng = np.random.default_rng(h * 1000 + w)
    p = Probe()
    dst = p.output((n, H, W, 3))
    dst2 = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    if entry.startswith("rgb"):
        real = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        src, src2 = p.input(real, rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)), torch.from_numpy(real).cuda()
        want = resize_model.resize(real, (H, W))

        def call(st, s=src, d=dst):
            ok(native, L.iiv_resize_frames(n, h, w, _dp(s), h * w * 3, w * 3, H, W, _dp(d), st))
        warm = lambda: call(native.stream_ptr(), src2, dst2)
    else:
        ch, cw = (h + 1) // 2, (w + 1) // 2
        ry = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
        ru, rv = rng.integers(0, 256, (2, n, ch, cw), dtype=np.uint8)
        want = resize_model.resize(yuv_model.to_rgb(ry, ru, rv, "bt601"), (H, W))
        m = p.host(np.asarray(yuv_model.MATRICES["bt601"], np.int32), np.asarray(yuv_model.MATRICES["jpeg"], np.int32))
        m2 = np.asarray(yuv_model.MATRICES["bt601"], np.int32)
        y, y2 = p.input(ry, np.roll(ry, 1, axis=0)), torch.from_numpy(ry).cuda()
        if entry == "i420":
            u, v = p.input(ru, np.roll(ru, 1, axis=0)), p.input(rv, np.roll(rv, 1, axis=0))
            u2, v2 = torch.from_numpy(ru).cuda(), torch.from_numpy(rv).cuda()
            planes, planes2, ps = (y, u.data_ptr(), v.data_ptr()), (y2, u2.data_ptr(), v2.data_ptr()), 1
        else:
            ruv = np.ascontiguousarray(np.stack([ru, rv], axis=-1))
            uv, uv2 = p.input(ruv, np.roll(ruv, 1, axis=0)), torch.from_numpy(ruv).cuda()
            planes, planes2, ps = (y, uv.data_ptr(), uv.data_ptr() + 1), (y2, uv2.data_ptr(), uv2.data_ptr() + 1), 2

        def call(st, pl=planes, d=dst, mat=m):
            ok(native, L.iiv_resize_frames_yuv420(n, h, w, _dp(pl[0]), h * w, w, C.c_void_p(pl[1]), C.c_void_p(pl[2]), ch * cw * ps, cw * ps,
                                                  ps, _hp(mat), H, W, _dp(d), st))
        warm = lambda: call(native.stream_ptr(), planes2, dst2, m2)
    # (the tables go up with blocking copies on the null stream: with the null stream asleep for longer than the side stream,
    # a copy that the call did not wait for lands after the kernels on the side stream have read the table)
    p.run(call, asynchronous=False, null_sleep=2 * SLEEP_CYCLES)
    warm()
    torch.cuda.synchronize()
    return _np(dst), _np(dst2), want


@pytest.mark.parametrize("case", CC.RESIZE_CASES, ids=[c[0] for c in CC.RESIZE_CASES])
def test_cold_resize_tables_on_a_sleeping_stream(native, case):
    """Case 7.  The first use of a size pair in the process makes its coefficient tables on the host and uploads them with
    blocking copies on the null stream (csrc/iiv_resize.hip get_table: hipMemcpy x 3) in front of a launch on `st` -- a host
    wait, so no `busy`.  The side stream sleeps and, behind the probe's marker, the null stream sleeps twice as long: the
    kernels may not start before the upload is complete.  The second, warm call of the pair gives the same bytes."""
    entry, h, w, H, W = case
    got, again, want = _cold_resize(native, entry, h, w, H, W)
    assert np.array_equal(got, want), "cold call: first difference at %s" % (np.argwhere(got != want)[:1],)
    assert np.array_equal(again, want), "warm call"


# ---- case 8: the shared form's first launch of a process, in a fresh child each ---------------------------------------------

CHILD_TIMEOUT = 120      # seconds; a child takes a few (interpreter, torch, the library, the tables)
_child_failed = []       # a child that ended abnormally: no further child is started in this process


@pytest.mark.parametrize("fourth", [False, True], ids=["three-offsets", "fourth-offset"])
@pytest.mark.parametrize("mode", MODES)
def test_cold_shared_form_in_a_fresh_process(O, oracle_tables, mode, fourth):
    """Case 8.  csrc/iiv_greedy.hip launch_shared sets resident_of[dev] and the kernel's LDS attribute at an instantiation's
    first launch of the process (host only, under a mutex); here that launch is an iiv_encode on a sleeping non-blocking stream,
    the child's first shared-form work, behind a priming call under the plain form (tests/cold_shared_child.py).  One child at a time, each under its own timeout, none started after one that
    ended abnormally; the four (mode, fourth-offset) instantiations."""
    assert not _child_failed, "an earlier child ended abnormally (%s): none is started after it" % _child_failed
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(cold_shared_child.__file__), str(mode), str(int(fourth))],
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env)
    except subprocess.TimeoutExpired:
        _child_failed.append("timeout")
        raise
    if r.returncode != 0:
        _child_failed.append("exit status %d" % r.returncode)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("cold-shared ")][-1].split(" ", 2)
    forms, busy = line[2].rsplit(" ", 1)
    fm, fa, segments = cold_shared_child.inputs(mode)
    n, s0 = cold_shared_child.N_STREAMS, cold_shared_child.SEED0
    prime = cold_shared_child.PRIME
    assert len(prime) == len(segments) == CC.CHILD_SEGMENTS
    want = np.stack([H.oracle_run(O, oracle_tables, mode, 5, np.stack([fm[i], fa[i]], axis=1), prime + segments, (s0 + i, s0 + 100 + i),
                                  fourth=fourth)[1][sum(g[3] for g in prime):] for i in range(n)])
    assert line[1] == cold_shared_child.digest(want)
    assert forms == '{"plain": 0, "shared": 3, "team": 0, "workgroup": 0}' and busy == "1", line


# ---- case 9: two encoders, each on its own sleeping stream, call by call ---------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_two_encoders_interleaved(native, O, device_tables, oracle_tables, mode):
    """Case 9.  X runs case 1's grow sequence, Y case 3's ring sequence (with stream 1 set in between), each on its own
    independent stream behind its own sleep, the calls alternating: different encoders are independent (include/iivision.h), so
    a staging buffer, ring or event that two of them shared would show.  (Both sequences wait on the host: no `busy`.)"""
    import torch
    x = Enc(native, O, device_tables, oracle_tables, mode, 2, 171)
    y = Enc(native, O, device_tables, oracle_tables, mode, 2, 181)
    cx, cy = Calls(native, x, 1460 + mode), Calls(native, y, 1470 + mode)
    assert cx.p.side.cuda_stream != cy.p.side.cuda_stream
    sx, check_x = _grow_sequence(cx)
    sy, check_y = _ring_sequence(cy, O, 7100, CC.RING_STREAM_1)
    torch.cuda.synchronize()
    cx.p.begin(synchronize=False)
    cy.p.begin(synchronize=False)
    stx, sty = C.c_void_p(cx.p.side.cuda_stream), C.c_void_p(cy.p.side.cuda_stream)
    for a, b_ in itertools.zip_longest(sx, sy):
        if a:
            a(stx)
        if b_:
            b_(sty)
    cx.p.end(asynchronous=False)
    cy.p.end(asynchronous=False)
    check_x("X, grow")
    check_y("Y, ring")
    x.close()
    y.close()
