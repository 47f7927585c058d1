"""CPU: what tests/test_gpu_cold_paths.py stands on, without a device.  The growth rules and ring sizes that
tests/cold_cases.py mirrors are read back from the text of csrc/; plain arithmetic on the mirrored constants shows that every
sequence crosses the boundary it is named after -- a changed constant fails here instead of quietly turning a grow case into a
steady-state one --; and the size pairs reserved for the cold resize tables are used by nothing else in tests/ and tools/, the
committed fuzz rounds included."""
import os
import re

import cold_cases as CC
import stage_fuzz as F

HERE = os.path.dirname(os.path.abspath(__file__))


def _src(name):
    with open(os.path.join(CC.CSRC, name)) as f:
        return f.read()


def _function(text, head):
    """the text of the function that starts with `head`, up to the closing brace in column 0"""
    at = text.index(head)
    return text[at:text.index("\n}\n", at)]


def test_mirrored_constants_are_the_sources():
    header, encode, encoder = _src("iiv_encoder.h"), _src("iiv_encode.hip"), _src("iiv_encoder.hip")
    assert int(re.search(r"constexpr int kSmallSlots = (\d+);", header).group(1)) == CC.K_SMALL_SLOTS
    assert int(re.search(r"HostBuf<LaunchSeg> h_segs\[(\d+)\];", header).group(1)) == CC.SEG_RING_SLOTS == 2
    up = _function(encode, "static int upload_segs(")
    assert "e->seg_slot ^= 1;" in up                                   # (two slots, taken in turn)
    assert int(re.search(r"e->d_segs\.alloc\((\d+) \* n,", up).group(1)) == CC.SEGS_GROWTH
    assert int(re.search(r"e->h_segs\[k\]\.alloc\((\d+) \* n,", up).group(1)) == CC.SEG_SLOT_GROWTH
    assert "if (n > e->d_segs.count())" in up and "if (n > e->h_segs[k].count())" in up
    rq = _function(encode, "static int reset_queues(")
    assert int(re.search(r"e->d_queue\.alloc\(n_rounds \* (\d+),", rq).group(1)) == CC.QUEUE_GROWTH
    assert "if (n_rounds > e->d_queue.count())" in rq and "zeroed_queue" in rq
    # the waits the GPU cases rest on stand in front of what they guard
    assert up.index("hipStreamSynchronize(st)") < up.index("e->d_segs.alloc(")
    assert up.index("hipEventSynchronize(e->seg_ev[k])") < up.index("e->h_segs[k].alloc(") < up.index("memcpy(e->h_segs[k]")
    assert rq.index("hipStreamSynchronize(st)") < rq.index("e->d_queue.alloc(") < rq.index("hipMemsetAsync(e->d_queue")
    ring = _function(encoder, "int encoder_set_state_async(")
    assert ring.index("hipEventSynchronize(e->small_ev[k])") < ring.index("memcpy(slot, buf, bytes)") < ring.index("hipEventRecord(e->small_ev[k], st)")
    assert "% kSmallSlots" in ring and "e->small_slot = -kSmallSlots;" in ring
    # iiv_encode: one descriptor and one counter per round (= per segment that emits)
    enc = _function(encode, "int encode(Encoder *e,")
    assert "upload_segs(e, rounds, st)" in enc and "reset_queues(e, rounds.size(), st)" in enc


def test_the_grow_sequence_crosses_every_boundary_it_names():
    p, a, b, c = CC.GROW_CALLS
    assert (p,) + CC.GROW_SEGMENTS == CC.GROW_CALLS and p == CC.PRIME_SEGMENTS
    d_segs = CC.capacities(CC.GROW_CALLS, CC.SEGS_GROWTH)
    assert d_segs[0] == 0 < p                                           # a fresh encoder holds nothing: the priming call grows
    assert a <= d_segs[1] == CC.SEGS_GROWTH * p                         # ... so that A, behind the sleep, does NOT: A sleeps
    assert b > d_segs[2] == d_segs[1]                                   # B is the first grow behind work in flight
    assert c > d_segs[3] == CC.SEGS_GROWTH * b                          # ... and C exceeds what B left
    slots = CC.seg_slots(CC.GROW_CALLS)
    assert slots[1] == (1, 0)                                           # A takes a slot nothing used: no event to wait for
    assert slots[2] == (0, CC.SEG_SLOT_GROWTH * p) and b > slots[2][1]  # B the primed one, too small (its copy long done)
    assert slots[3][0] == slots[1][0] and c > slots[3][1] == CC.SEG_SLOT_GROWTH * a > 0   # C takes A's, too small, a copy to wait for
    d_queue = CC.capacities(CC.GROW_CALLS, CC.QUEUE_GROWTH)             # (rounds of an iiv_encode call = its emitting segments)
    assert a <= d_queue[1] == CC.QUEUE_GROWTH * p and b > d_queue[2] and c > d_queue[3]
    # case 8's child: its priming call leaves room for the cold call's descriptors and counters, in a slot of its own
    child = (CC.CHILD_SEGMENTS, CC.CHILD_SEGMENTS)
    assert CC.capacities(child, CC.SEGS_GROWTH)[1] >= CC.CHILD_SEGMENTS <= CC.capacities(child, CC.QUEUE_GROWTH)[1]
    assert CC.seg_slots(child)[1] == (1, 0)
    # the two-encode sequences behind a priming call of one segment (cases 3-6: at most two segments a call) never grow d_segs
    assert CC.capacities((p, 2, 2), CC.SEGS_GROWTH) == [0, 2, 2]
    for mode in (0, 1):
        for j, n in enumerate(CC.GROW_SEGMENTS):
            segs = CC.grow_segments(mode, n, j)
            assert len(segs) == n and segs[0][2] == 1 and all(24 <= s[3] <= 48 for s in segs)
            assert all(s[0] in (0, 1) and s[1] in ((0, 1) if mode else (0,)) for s in segs)
            for prev, s in zip(segs, segs[1:]):                         # a continued generator keeps its frame and bank
                assert s[2] == 1 or s[:2] == prev[:2]
    # the mirror itself: a steady-state sequence does not grow
    assert CC.capacities((3, 3, 3), 2) == [0, 6, 6] and CC.seg_slots((3, 3, 3)) == [(0, 0), (1, 0), (0, 6)]


def test_the_ring_sequence_wraps_and_every_last_write_matters():
    assert CC.RING_CALLS == CC.K_SMALL_SLOTS + 3 > CC.K_SMALL_SLOTS
    slots = CC.small_slots(CC.RING_CALLS)
    assert [s for s, _ in slots[:CC.K_SMALL_SLOTS]] == list(range(CC.K_SMALL_SLOTS)) and not any(w for _, w in slots[:CC.K_SMALL_SLOTS])
    assert all(w for _, w in slots[CC.K_SMALL_SLOTS:]) and slots[CC.K_SMALL_SLOTS][0] == 0
    for stream_1 in ((), CC.RING_STREAM_1):
        plan = CC.ring_plan(stream_1)
        assert {k for k, s in plan if s == 0} == set(CC.RING_KINDS)      # stream 0 has all three items set
        assert len(plan) == CC.RING_CALLS
    # With every call on stream 0 each first-round write is set again later (the issue's sequence): that case holds the final
    # state and the ring's advance, and cannot see a missing wait.  The variant can: stream 1's items are each set once, so a
    # write that a later call's bytes replaced in its slot, while it was still queued, reaches the final state -- two of them sit
    # in slots that are taken again, by a call of ANOTHER item, one of them the 8-byte item under a 2500-byte one
    plan = CC.ring_plan(CC.RING_STREAM_1)
    kinds_1 = [plan[i][0] for i in CC.RING_STREAM_1]
    assert sorted(kinds_1) == sorted(CC.RING_KINDS)
    reused = [i for i in CC.RING_STREAM_1 if i + CC.K_SMALL_SLOTS < CC.RING_CALLS]
    assert len(reused) == 2 and len(CC.RING_STREAM_1) == 3
    for i in reused:
        assert plan[i + CC.K_SMALL_SLOTS][0] != plan[i][0] and plan[i + CC.K_SMALL_SLOTS][1] == 0
    assert ("OUT_OF_WORK", "RNG_PY") in [(plan[i][0], plan[i + CC.K_SMALL_SLOTS][0]) for i in reused]


def _numbers(path):
    with open(path, errors="replace") as f:
        return set(int(x) for x in re.findall(r"(?<![\w.])\d+(?![\w.])", f.read()))


def test_the_reserved_resize_pairs_are_used_nowhere_else():
    """What this covers: numbers written out in the files of tests/ and tools/ (the listed extensions) and the committed rounds of
    stage_fuzz.  It does not cover sizes drawn at run time (tests/fuzz_parity.py and tests/long_parity.py draw no resize shapes
    today) or computed in loops."""
    cases = CC.RESIZE_CASES
    assert [c[0] for c in cases] == ["rgb_one_pass", "rgb_two_pass", "i420", "nv12"]
    _, h, w, H, W = cases[0]
    assert h == H and w != W                                             # one pass: the width alone
    assert all(c[1] != c[3] and c[2] != c[4] for c in cases[1:])         # two passes
    pairs = [p for c in cases for p in CC.axis_pairs(c)]
    assert len(set(pairs)) == len(pairs) == 8
    assert all(h % 2 and w % 2 and H % 2 and W % 2 and 1 <= H <= 1024 and 1 <= W <= 1024 for _, h, w, H, W in cases)
    # every resized axis starts from a source size that occurs as a number in no other file of tests/ and tools/
    sources = {i for i, o in pairs if i != o}
    assert len(sources) == 7
    own = {"cold_cases.py"}
    for top in ("tests", "tools"):
        for d, _, names in os.walk(os.path.join(CC.ROOT, top)):
            for name in names:
                if name in own or not name.endswith((".py", ".sh", ".hip", ".h", ".c", ".cpp", ".txt", ".json")):
                    continue
                hit = sources & _numbers(os.path.join(d, name))
                assert not hit, "%s names %s" % (os.path.join(d, name), sorted(hit))
    # ... and the committed fuzz rounds draw none of the pairs
    reserved = set(pairs)
    seen = 0
    for stage in F.STAGES:
        for r in range(F.ROUNDS[stage]):
            p = F.DRAW[stage](F.stage_rng(F.SEED, r, stage), r).get("params", {})
            if all(k in p for k in ("h", "w", "H", "W")):
                seen += 1
                assert not {(p["h"], p["H"]), (p["w"], p["W"])} & reserved, (stage, r, p)
    assert seen >= F.ROUNDS["resize"] + F.ROUNDS["yuv"]
