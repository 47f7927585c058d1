"""GPU: a live generator handed from one greedy kernel form to another.  Every other encode test sets the
greedy kernel once per encoder, so a generator is only ever continued by the form that created it; here each launch of a
generator runs under the form its plan names (tests/form_handover.py; its conditions: test_form_handover_host.py), and what
one form wrote back -- list position, pushed keys, the primaries' bits, random's MT19937 block and its index, the 16-bit
priorities -- is what the next one loads.  Byte-exact: stream 0 of a case against the reference's recording
(tests/golden/g11_reference_corpus.npz), every stream against the oracle.  Every case counts its launches by kernel
(launch_forms): one that silently ran a single form fails."""
import collections

import numpy as np
import pytest

import encode_harness as H
import form_handover as FH
import reference_corpus as RC

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def corpus(golden):
    return RC.load(golden)


def _encoder(native, O, device_tables, rec, seeds, recurrence=True):
    mode, pal, _, _, fourth, _ = (int(x) for x in rec["meta"])
    enc = H.make_encoder(native, device_tables, mode, pal, len(seeds), dw=recurrence, rng=seeds, O=O,
                         **({"fourth": True} if fourth else {}))
    enc.profile(True)
    return enc


def _ran(launches, fourth):
    """launch_forms() as the plan wants it: with the fourth offset a requested "workgroup" runs the plain one-wave kernel"""
    want = dict.fromkeys(FH.FORMS, 0)
    for L in launches:
        want["plain" if fourth and L.form == "workgroup" else L.form] += 1
    return want


def _run(enc, fm, fa, launches, between=None):
    """every launch under its form; between(i): called in front of launch i.  Returns (n_streams, total, 6) uint8."""
    import torch
    out = []
    for i, L in enumerate(launches):
        if between is not None:
            between(i)
        enc.set_greedy_kernel(L.form)
        out.append(enc.encode(fm, fa, [(L.frame, L.is_aux, L.restart, L.chunk)]))
    enc.check()
    return torch.cat(out, dim=1).cpu().numpy()


def _where(launches, pos):
    L = [x for x in launches if x.pos <= pos][-1]
    before = launches[launches.index(L) - 1].form if not L.restart else "(new generator)"
    return "opcode %d, in launch %d-%d under %r after %r" % (pos, L.pos, L.pos + L.chunk, L.form, before)


def _check_ops(tag, rec, got, streams, launches):
    bad = H.first_difference(got[0], rec["ops"], tag)
    assert bad is None, "%s stream 0 leaves the recording at %s: got %s want %s" % (tag, _where(launches, bad), got[0][bad], rec["ops"][bad])
    for i, e in enumerate(streams):
        bad = H.first_difference(got[i], e.ops, "%s stream %d" % (tag, i))
        assert bad is None, "%s stream %d leaves the oracle at %s: got %s want %s" % (tag, i, _where(launches, bad), got[i][bad], e.ops[bad])


def _check_state(native, tag, rec, enc, streams):
    """the shared state check (both generators in full: every draw behind the last launch, through the end of the block and
    into the next) and all four counters, behind the last launch"""
    mode, segs = int(rec["meta"][0]), FH.segments(rec)
    for i, e in enumerate(streams):
        v, what = e.video, "%s stream %d" % (tag, i)
        H.check_oracle_state(native, enc, i, v, mode, what)
        pad = sum(int(RC.is_padding(e.ops[s:s + n], rec["frames"], fi, ia).sum()) for (fi, ia, s, n, _) in segs)
        assert [int(x) for x in enc.get_state(native.STATE_COUNTERS, i)] == list(v.draws()) + [len(e.ops), pad], what


@pytest.mark.parametrize("recurrence", [True, "split"])
@pytest.mark.parametrize("tag", FH.BASE_CASES)
def test_the_matrix(native, O, corpus, device_tables, tag, recurrence):
    """A. Every ordered pair of forms hands every long generator of the case over, in each quarter of its real opcodes and
    in its padding; 9 (DHGR) or 17 (HGR) streams, one full and one partly filled workgroup of the shared form.  One encoder;
    per launch set_greedy_kernel(form), then encode() of one segment.  The two diff-weight modes start the walk at
    different places (form_handover.STARTS), so that over both every form also creates a generator.  Opcodes, the state
    behind the last launch, and the launches counted by kernel are what the plan says."""
    rec = corpus[tag]
    fourth = bool(rec["meta"][4])
    launches = FH.plan(rec["schedule"], FH.forms_of(rec), start=FH.STARTS[0 if recurrence is True else 1])
    streams = FH.expected(tag, rec)
    enc = _encoder(native, O, device_tables, rec, FH.batch(rec), recurrence)
    fm, fa = H.device_frames(int(rec["meta"][0]), [rec["frames"]] * len(streams))
    got = _run(enc, fm, fa, launches)
    ran = enc.launch_forms()
    print("%s, diff weights %r: %d launches, %d hand-overs, by kernel %s" % (tag, recurrence, len(launches), len(FH.handovers(launches)), ran))
    assert ran == _ran(launches, fourth) and all(ran[f] > 0 for f in FH.forms_of(rec)) and (ran["workgroup"] == 0) == fourth, ran
    _check_ops(tag, rec, got, streams, launches)
    _check_state(native, tag, rec, enc, streams)
    enc.close()


@pytest.mark.parametrize("tag", ["HGR_static_exhaust", "DHGR_static_exhaust_iigs"])
def test_the_host_looks_in_between(native, O, corpus, device_tables, tag):
    """B. A's plan again, the host reading both banks' priorities in front of every tenth hand-over: the 16-bit priorities
    one form left are written out in full for the host (materialise_up_kernel) and compacted again (compact_up_kernel) for the
    form that follows.  Streams 0, the last of the full workgroup and the last are compared there, against an oracle pulled
    in step; every stream's opcodes are compared at the end.  HGR_static_exhaust's later generators stack priorities."""
    rec = corpus[tag]
    mode = int(rec["meta"][0])
    launches = FH.plan(rec["schedule"], FH.forms_of(rec), start=FH.STARTS[0])
    streams, seeds = FH.expected(tag, rec), FH.batch(rec)
    look_at = sorted({0, len(seeds) - 2, len(seeds) - 1})
    tenth = {i for k, (i, _, _, _) in enumerate(FH.handovers(launches)) if k % 10 == 0}
    differ = {i for (i, _, a, b) in FH.handovers(launches) if i in tenth and a != b}
    assert len(tenth) >= 15 and len(differ) >= 8
    videos = {s: RC.oracle_video(FH._Seeded(rec, seeds[s])) for s in look_at}
    enc = _encoder(native, O, device_tables, rec, seeds)
    fm, fa = H.device_frames(mode, [rec["frames"]] * len(streams))
    looked = []

    def between(i):
        if i > 0:       # the oracles catch up with launch i - 1
            L = launches[i - 1]
            for v in videos.values():
                if L.restart:
                    v.encode_frame(rec["frames"][L.frame, 0], rec["frames"][L.frame, 1] if mode else None, L.is_aux)
                v.next(L.chunk)
        if i in tenth:
            for s, v in videos.items():
                for b in range(mode + 1):
                    got = enc.get_state((native.STATE_UP_MAIN, native.STATE_UP_AUX)[b], s)
                    assert (got == v.update_priority(b)).all(), "%s stream %d bank %d in front of launch %d (%s)" % (tag, s, b, i, launches[i].form)
            looked.append(i)

    got = _run(enc, fm, fa, launches, between)
    assert len(looked) == len(tenth)
    assert enc.launch_forms() == _ran(launches, False)
    _check_ops(tag, rec, got, streams, launches)
    enc.close()


@pytest.mark.parametrize("tag", ["HGR_static_exhaust_fourth", "DHGR_static_exhaust_iigs_fourth"])
def test_the_fallback_is_a_handover_too(native, O, corpus, device_tables, tag):
    """C. With the fourth offset a requested "workgroup" runs the plain one-wave kernel (iiv_launch_choice.h).  The walk over
    all four names: the same bytes, no workgroup launch, and the launches asked of "workgroup" counted under "plain"."""
    rec = corpus[tag]
    launches = FH.plan(rec["schedule"], FH.FORMS)
    assert sum(L.form == "workgroup" for L in launches) >= 40
    streams = FH.expected(tag, rec)
    enc = _encoder(native, O, device_tables, rec, FH.batch(rec))
    fm, fa = H.device_frames(int(rec["meta"][0]), [rec["frames"]] * len(streams))
    got = _run(enc, fm, fa, launches)
    ran = enc.launch_forms()
    assert ran == _ran(launches, True) and ran["workgroup"] == 0 and min(ran["plain"], ran["shared"], ran["team"]) > 0, ran
    _check_ops(tag, rec, got, streams, launches)
    _check_state(native, tag, rec, enc, streams)
    enc.close()


@pytest.mark.parametrize("swapped", [False, True])
def test_one_call_two_forms(native, O, corpus, device_tables, swapped):
    """D. One encode_streams call of a DHGR encoder on "shared", 9 streams in two groups on DHGR_img_exhaust's frames.  Group X
    (the even streams) pulls one generator in four segments, group Y (the odd ones) starts a generator per round, on the
    other bank in rounds 1 and 3: those rounds mix banks and run the plain form, rounds 2 and 4 the shared one -- X's
    generator goes plain -> shared -> plain -> shared inside the call.  The cuts are taken from stream 0's generator: 37
    opcodes in, in its last quarter, and at its last real opcode, so that the fourth launch finds the list dry by itself
    (the other streams' generators end a few opcodes earlier or later).  swapped: X on aux, Y's banks exchanged."""
    tag = "DHGR_img_exhaust"
    rec = corpus[tag]
    frames, seeds = rec["frames"], FH.batch(rec)
    bx = 1 if swapped else 0
    if swapped:     # (not a generator of the recording: its length comes from the oracle)
        v = RC.oracle_video(FH._Seeded(rec, seeds[0]))
        v.encode_frame(frames[0, 0], frames[0, 1], bx)
        real = int(np.nonzero(~RC.is_padding(v.next(RC.MAX_OPS), frames, 0, bx))[0].max()) + 1
    else:
        real = FH.segments(rec)[0][4]
    assert 2000 < real < 4000
    cuts = [0, 37, real * 7 // 8, real, real + 24]
    sched_x = [(0, bx, 1 if k == 0 else 0, cuts[k + 1] - cuts[k]) for k in range(4)]
    sched_y = [(0, 1 - bx, 1, 50), (1, bx, 1, 121), (1, 1 - bx, 1, 90), (1, bx, 1, 200)]
    scheds = [sched_x if s % 2 == 0 else sched_y for s in range(len(seeds))]
    enc = _encoder(native, O, device_tables, rec, seeds)
    enc.set_greedy_kernel("shared")
    fm, fa = H.device_frames(1, [frames] * len(seeds))
    ops, totals = enc.encode_streams(fm, fa, scheds)
    enc.check()
    ran = enc.launch_forms()
    assert ran == {"plain": 2, "shared": 2, "team": 0, "workgroup": 0}, ran
    got = ops.cpu().numpy()
    for s, (sp, sn) in enumerate(seeds):
        v = RC.oracle_video(FH._Seeded(rec, (sp, sn)))
        want = []
        for (f, a, r, k) in scheds[s]:
            if r:
                v.encode_frame(frames[f, 0], frames[f, 1], a)
            want.append(v.next(k))
        want = np.concatenate(want)
        assert totals[s] == len(want)
        bad = H.first_difference(got[s, :totals[s]], want, "stream %d" % s)
        assert bad is None, "stream %d (group %s) leaves the oracle at opcode %d of %s" % (s, "XY"[s % 2], bad, [g[3] for g in scheds[s]])
        assert not got[s, totals[s]:].any()
        H.check_oracle_state(native, enc, s, v, 1, "stream %d" % s)
    if not swapped:
        assert (got[0, :totals[0]] == rec["ops"][:totals[0]]).all()
    enc.close()


def test_snapshot_under_one_form_roll_back_into_another(native, O, corpus, device_tables):
    """E. DHGR_static_exhaust_iigs, its long generator under "plain"; then snapshot(), 300 opcodes under "team", rollback(),
    the same 300 under "workgroup", rollback(), and under "shared": three times the oracle's next 300.  Once through slot 1
    in the middle of the generator, once through slot 0 from 280 opcodes before stream 0's last real one: pushed[] is at its
    fullest there, and the 300 run the list dry, walk the bag, come out of work and pad.  (The bag never yields an opcode
    in the reference's order: a pushed byte still has its list entry in front of it.  Walking it is what ends a generator.)"""
    tag = "DHGR_static_exhaust_iigs"
    rec = corpus[tag]
    seeds, streams = FH.batch(rec), FH.expected(tag, rec)
    (f, a, start, n, real) = FH.segments(rec)[2]
    assert n > 4000 and n - real >= 20
    enc = _encoder(native, O, device_tables, rec, seeds)
    fm, fa = H.device_frames(1, [rec["frames"]] * len(seeds))
    enc.set_greedy_kernel("plain")
    enc.encode(fm, fa, H.segments(rec["schedule"][:2]))
    pos, want_forms = 0, collections.Counter(plain=2)
    for slot, at in ((1, real // 2), (0, real - 280)):
        enc.set_greedy_kernel("plain")
        enc.encode(fm, fa, [(f, a, 1 if pos == 0 else 0, at - pos)])
        want_forms["plain"] += 1
        enc.snapshot(slot)
        runs = {}
        for form in ("team", "workgroup", "shared"):
            if runs:
                enc.rollback(slot)
            enc.set_greedy_kernel(form)
            runs[form] = enc.encode(fm, fa, [(f, a, 0, 300)]).cpu().numpy()
            want_forms[form] += 1
        enc.check()
        for form, ops in runs.items():
            for s, e in enumerate(streams):
                bad = H.first_difference(ops[s], e.ops[start + at:start + at + 300], "slot %d, %r, stream %d" % (slot, form, s))
                assert bad is None, "slot %d, %r from opcode %d: stream %d differs at +%d" % (slot, form, at, s, bad)
        pos = at + 300
    assert pos == real + 20
    padded = RC.is_padding(runs["shared"][0], rec["frames"], f, a)
    assert padded[-20:].all() and not padded[:280].any()
    assert enc.launch_forms() == {k: want_forms[k] for k in FH.FORMS}
    enc.close()


@pytest.mark.parametrize("tag", ["HGR_img_exhaust", "DHGR_img_exhaust"])
def test_live_and_back(native, O, corpus, device_tables, tag):
    """F. A one-stream encoder, the case cut as its plan cuts it; the launches alternate between encode_live (the team
    kernel; slot 0 / 1 in turn, the tag counting up) and encode under "plain", "workgroup" and "shared" in turn -- what the
    drop-in Video does when it leaves the live path and comes back.  d_ops_out is the recording.  (The queue's own contract:
    test_live_queue_carries_every_opcode.)"""
    import torch
    rec = corpus[tag]
    mode = int(rec["meta"][0])
    cuts = FH.plan(rec["schedule"], FH.FORMS)
    others = ("plain", "workgroup", "shared")
    launches = [L._replace(form="team" if i % 2 == 0 else others[(i // 2) % 3]) for i, L in enumerate(cuts)]
    enc = _encoder(native, O, device_tables, rec, FH.batch(rec)[:1])
    fm, fa = H.device_frames(mode, [rec["frames"]])
    enc.live_queue(0), enc.live_queue(1)
    buf = torch.empty((1, 128, 6), dtype=torch.uint8, device="cuda")
    out = []
    for i, L in enumerate(launches):
        enc.set_greedy_kernel(L.form)
        if L.form == "team":
            enc.encode_live(fm, fa, (L.frame, L.is_aux, L.restart, L.chunk), buf, (i // 2) & 1, 1 + i // 2)
            out.append(buf[:, :L.chunk].clone())
        else:
            out.append(enc.encode(fm, fa, [(L.frame, L.is_aux, L.restart, L.chunk)]))
    enc.check()
    assert enc.launch_forms() == _ran(launches, False) and min(enc.launch_forms().values()) >= 30
    got = torch.cat(out, dim=1).cpu().numpy()
    bad = H.first_difference(got[0], rec["ops"], tag)
    assert bad is None, "%s leaves the recording at %s" % (tag, _where(launches, bad))
    _check_state(native, tag, rec, enc, FH.expected(tag, rec)[:1])
    enc.close()
