"""Hand-over plans: a live generator continued by another greedy kernel form than the one that left it.

The four greedy kernels -- the one-wave kernel in its plain and its LDS-shared form, the eight-wave team kernel and the
workgroup kernel -- each load and write back the generator's record in StreamState in their own way.  A plan cuts every
generator of a corpus case (reference_corpus.Case.schedule(): (frame, is_aux, n_ops)) into launches and names the kernel
to set before each, so that every ordered pair of forms hands a generator over, in every phase of its life.  No device is
used here: test_form_handover_host.py checks the plans' conditions with the oracle alone, test_gpu_form_handover.py runs
them.

    plan(schedule, forms)        [Launch]: the launches of one case
    handovers(launches)          [(launch index, opcode position, form before, form after)]
    batch(rec)                   the seeds of the case's streams (stream 0: the recording's own)
    expected(tag, rec, launches) per stream: the oracle's opcodes, its draw count at every cut, the Video as it ends
"""
import collections

import numpy as np

import reference_corpus as RC

FORMS = ("plain", "shared", "team", "workgroup")
FORMS_FOURTH = ("plain", "shared", "team")       # with the fourth offset "workgroup" runs the one-wave kernel (iiv_launch_choice.h)
# 13 sizes, coprime to both walks (16 and 9 transitions).  Not the first cycle tried (1 2 3 5 8 13 21 34 55 89 64 65 127, mean
# 37): with it a quarter of DHGR_img_exhaust's second generator (582 opcodes) holds fewer than the 16 cuts it must show.  This
# one has the same edges -- one, two and three opcodes, a wave's 64 and one more, 127 -- a mean of 31, and no three
# neighbours above 165, so that 16 consecutive cuts span at most 567 opcodes.
CHUNKS = (127, 1, 2, 65, 3, 5, 64, 8, 13, 55, 21, 4, 34)
# A generator longer than TAIL_MIN ends in TAIL launches of one opcode: the 24 padding opcodes the exhaustion cases pull
# behind a generator's last real one are the only place where both sides of a cut are padding, and every pair has to fit.
TAIL, TAIL_MIN = 23, 200
BASE_CASES = ("HGR_img_exhaust", "DHGR_img_exhaust", "HGR_static_exhaust", "DHGR_static_exhaust_iigs",
              "HGR_static_exhaust_fourth", "DHGR_static_exhaust_iigs_fourth")
N_STREAMS = {RC.HGR: 17, RC.DHGR: 9}       # one full and one partly filled workgroup of the shared form (16 / 8 streams)
# (seed_py, seed_np) of streams 1 .. 16, every case; stream 0 has the recording's.
SEEDS = tuple((7001 + 13 * i, 9001 + 17 * i) for i in range(16))

# Where the walk starts in the two plans test_the_matrix runs of a case (one per diff-weight mode).  A case has three to five
# generators and DHGR_static_exhaust_iigs creates its second and third under one form whatever the start, so no single plan
# lets all four forms create one; with these two starts every case has a generator created by each form.
STARTS = (3, 6)
# What test_handovers_meet_the_mt_block_edges counts over every stream, case and plan, by receiving form: hand-overs with
# 1 .. 8 words of random's MT19937 block left, and with the block exactly used up (DESIGN.md 20 prints these)
MT_EDGE_HITS = {"near": {"plain": 103, "shared": 94, "team": 149, "workgroup": 50},
                "empty": {"plain": 16, "shared": 17, "team": 14, "workgroup": 13}}

Launch = collections.namedtuple("Launch", "gen frame is_aux restart chunk form pos")    # pos: the first opcode's index in the stream


def walk(forms):
    """A closed walk through every ordered pair of `forms`, self-pairs included, each once: the de Bruijn sequence B(k, 2)
    in its smallest (Lyndon word) order -- k * k forms, read as a cycle."""
    k, seq = len(forms), []

    def db(t, p, a):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p, a)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t, a)

    db(1, 1, [0] * 3)
    assert len(seq) == k * k
    pairs = {(seq[i], seq[(i + 1) % len(seq)]) for i in range(len(seq))}
    assert len(pairs) == k * k
    return tuple(forms[i] for i in seq)


def forms_of(rec):
    return FORMS_FOURTH if int(rec["meta"][4]) else FORMS


def plan(schedule, forms, the_walk=None, chunks=CHUNKS, start=0):
    """The launches of a case: launch i runs form walk[(start + i) % len] and asks for chunks[i % 13] opcodes, across
    generator boundaries; a generator's last chunk of the cycle is cut to fit, and a generator longer than TAIL_MIN ends in
    TAIL launches of one opcode.  `the_walk`: another closed walk (case C)."""
    w = the_walk or walk(forms)
    out, i, pos = [], 0, 0
    for g, (frame, is_aux, n_ops) in enumerate(schedule):
        tail = TAIL if n_ops > TAIL_MIN else 0
        done = 0
        while done < n_ops:
            k = 1 if done >= n_ops - tail else min(chunks[i % len(chunks)], n_ops - tail - done)
            out.append(Launch(g, int(frame), int(is_aux), 1 if done == 0 else 0, k, w[(start + i) % len(w)], pos))
            done, pos, i = done + k, pos + k, i + 1
    return out


def handovers(launches):
    """[(index of the receiving launch, opcode position of the cut, form that wrote the state, form that loads it)]"""
    return [(i, b.pos, a.form, b.form) for i, (a, b) in enumerate(zip(launches, launches[1:]), 1) if not b.restart]


def segments(rec):
    """[(frame, is_aux, first opcode, n_ops, real opcodes)] of a recording: `real` = up to its last opcode that is no padding"""
    out, pos = [], 0
    for fi, ia, n in rec["schedule"]:
        pad = RC.is_padding(rec["ops"][pos:pos + n], rec["frames"], int(fi), int(ia))
        real = np.nonzero(~pad)[0]
        out.append((int(fi), int(ia), pos, int(n), int(real.max()) + 1 if len(real) else 0))
        pos += int(n)
    return out


class _Seeded:
    """what reference_corpus.oracle_video reads of a Case"""

    def __init__(self, rec, seeds):
        self.mode, self.palette, _, _, fourth, _ = (int(x) for x in rec["meta"])
        self.seed_py, self.seed_np = seeds
        self.fourth = bool(fourth)


def batch(rec):
    """[(seed_py, seed_np)] of the case's streams"""
    mode, _, sp, sn = (int(x) for x in rec["meta"][:4])
    return [(sp, sn)] + list(SEEDS[:N_STREAMS[mode] - 1])


class Expected:
    """a stream as the oracle leaves it: its opcodes, random's draw count at every cut (by opcode position), the Video at the end"""

    def __init__(self, ops, draws, video):
        self.ops, self.draws, self.video = ops, draws, video

    def draws_at(self, pos):
        return self.draws[pos]


def oracle_stream(rec, seeds, launches):
    """the oracle driven launch by launch (chunking next() changes nothing: test_form_handover_host.py)"""
    v = RC.oracle_video(_Seeded(rec, seeds))
    frames, mode = rec["frames"], int(rec["meta"][0])
    ops, draws = [], {}
    for L in launches:
        if L.restart:
            v.encode_frame(frames[L.frame, 0], frames[L.frame, 1] if mode == RC.DHGR else None, L.is_aux)
        draws[L.pos] = v.draws()[0]
        ops.append(v.next(L.chunk))
    return Expected(np.concatenate(ops), draws, v)


_EXPECTED = {}


def expected(tag, rec, launches=None):
    """[Expected] per stream of case `tag`, cut as its plans cut it (the cuts do not depend on where the walk starts),
    computed once per process and shared by every test of the case."""
    if tag not in _EXPECTED:
        launches = launches or plan(rec["schedule"], forms_of(rec))
        _EXPECTED[tag] = [oracle_stream(rec, s, launches) for s in batch(rec)]
    return _EXPECTED[tag]
