"""What tests/test_gpu_cold_paths.py and tests/test_cold_paths_host.py share: the library's first-use and grow-on-demand rules,
mirrored with their source lines (the host file reads them back from csrc/ and fails if one moved), the call sequences that
cross them, and the arithmetic that says they do.  No device is touched here."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ii-vision_amd", "csrc")

K_SMALL_SLOTS = 4        # csrc/iiv_encoder.h: constexpr int kSmallSlots = 4 (iiv_encoder_set_state_async's staging ring)
SEGS_GROWTH = 2          # csrc/iiv_encode.hip upload_segs: e->d_segs.alloc(2 * n, ...)       when n > d_segs.count()
SEG_SLOT_GROWTH = 2      # csrc/iiv_encode.hip upload_segs: e->h_segs[k].alloc(2 * n, ...)    when n > h_segs[k].count()
SEG_RING_SLOTS = 2       # csrc/iiv_encoder.h: HostBuf<LaunchSeg> h_segs[2]; upload_segs: e->seg_slot ^= 1
QUEUE_GROWTH = 2         # csrc/iiv_encode.hip reset_queues: e->d_queue.alloc(n_rounds * 2, ...) when n_rounds > d_queue.count()

# iiv_encode takes one descriptor and one launch round per segment that emits opcodes.  A fresh encoder holds no descriptor
# buffer at all (d_segs.count() == 0), so its first encode grows from nothing and waits for its stream: every encoder case
# makes that first encode -- PRIME_SEGMENTS segments, on the idle null stream, synchronised, the oracle making it too -- BEFORE
# the sleep, and the sequence under test starts behind it.  The segments of the priming call P and of calls A, B, C of the grow
# sequence (cases 1, 2 and 9):
PRIME_SEGMENTS = 1
GROW_SEGMENTS = (1, 3, 7)
GROW_CALLS = (PRIME_SEGMENTS,) + GROW_SEGMENTS
RING_CALLS = K_SMALL_SLOTS + 3     # iiv_encoder_set_state_async calls between the two encodes of the ring sequence (cases 3, 9)
RING_KINDS = ("RNG_PY", "RNG_NP", "OUT_OF_WORK")
# the variant's calls that set stream 1, each item once and never again: RNG_NP (call 1) and OUT_OF_WORK (call 2) sit in slots
# that calls 5 and 6 take again for another item while the writes are still queued; RNG_PY (call 3) in a slot none takes again
RING_STREAM_1 = (1, 2, 3)
CHILD_SEGMENTS = 3       # case 8: rounds of the child's priming call (forced plain form) and of its cold shared call

# Case 7: (entry, h, w, H, W), each first used on the sleeping side stream.  No other test, tool or fuzz round resizes an
# axis from one of these source sizes (tests/test_cold_paths_host.py greps for them and recomputes the fuzz's rounds), so the
# coefficient tables of all eight axis pairs are cold whatever ran before in the process.
RESIZE_CASES = (("rgb_one_pass", 19, 347, 19, 83), ("rgb_two_pass", 349, 353, 59, 101),
                ("i420", 337, 419, 47, 67), ("nv12", 379, 383, 53, 71))


def axis_pairs(case):
    _, h, w, H, W = case
    return [(h, H), (w, W)]


def capacities(calls, growth):
    """a grow-on-demand buffer over a sequence of calls that need calls[i] elements -> its capacity BEFORE each call
    (alloc(growth * n) when n exceeds what is there, from nothing)"""
    cap, before = 0, []
    for n in calls:
        before.append(cap)
        if n > cap:
            cap = growth * n
    return before


def seg_slots(calls):
    """upload_segs' pinned ring over the same sequence -> (slot, its capacity before the call) per call"""
    cap, slot, out = [0] * SEG_RING_SLOTS, 0, []
    for n in calls:
        out.append((slot, cap[slot]))
        if n > cap[slot]:
            cap[slot] = SEG_SLOT_GROWTH * n
        slot = (slot + 1) % SEG_RING_SLOTS
    return out


def small_slots(n_calls, slots=K_SMALL_SLOTS):
    """encoder_set_state_async's ring -> (slot, does the call wait for the slot's event) per call"""
    return [(i % slots, i >= slots) for i in range(n_calls)]


def grow_segments(mode, n, call):
    """n segments (frame, is_aux, restart, n_ops) of two or three dozen opcodes each: generators restarted and continued, both
    frames, in DHGR both banks; the first of a call restarts"""
    out = []
    for j in range(n):
        f, a = ((j // 2) + call) % 2, ((j // 2) % 2 if mode == 1 else 0)
        out.append((f, a, 1 if j % 2 == 0 else 0, 24 + 5 * ((j + call) % 3)))
    return out


def ring_plan(stream_1=()):
    """the ring sequence -> (kind, stream) per call"""
    return [(RING_KINDS[i % 3], 1 if i in stream_1 else 0) for i in range(RING_CALLS)]
