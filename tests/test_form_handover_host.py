"""CPU: the conditions under which the hand-over plans of tests/form_handover.py show what they are for --
conditions on the INPUTS of test_gpu_form_handover.py, checked with the recordings and the oracle alone.  Where one fails
the chunk cycle, the walk or the seed table changes; the condition does not."""
import collections

import numpy as np
import pytest

import form_handover as FH
import reference_corpus as RC


@pytest.fixture(scope="module")
def corpus(golden):
    return RC.load(golden)


def _plans(rec):
    """the plans test_the_matrix runs of a case: one per diff-weight mode"""
    return [FH.plan(rec["schedule"], FH.forms_of(rec), start=s) for s in FH.STARTS]


def test_walks_are_closed_and_complete():
    """each walk goes through every ordered pair of its forms once, and its length is coprime to the chunk cycle's"""
    for forms in (FH.FORMS, FH.FORMS_FOURTH):
        w = FH.walk(forms)
        pairs = collections.Counter((w[i], w[(i + 1) % len(w)]) for i in range(len(w)))
        assert len(w) == len(forms) ** 2 and set(pairs.values()) == {1} and len(pairs) == len(forms) ** 2
        assert np.gcd(len(w), len(FH.CHUNKS)) == 1
    assert len(FH.CHUNKS) == 13 and min(FH.CHUNKS) == 1 and max(FH.CHUNKS) == 127 and {64, 65} <= set(FH.CHUNKS)
    assert len(set(FH.SEEDS)) == 16 and FH.N_STREAMS == {RC.HGR: 17, RC.DHGR: 9}


@pytest.mark.parametrize("tag", FH.BASE_CASES)
def test_plans_cut_the_recording(corpus, tag):
    """per generator the chunks sum to the schedule's n_ops, the first launch of a generator restarts and no other does, the
    case's total is the recording's length -- and the oracle pulled chunk by chunk gives the recording (stream 0)"""
    rec = corpus[tag]
    for launches in _plans(rec):
        per_gen = collections.defaultdict(list)
        for L in launches:
            per_gen[L.gen].append(L)
        assert len(per_gen) == len(rec["schedule"])
        for g, (fi, ia, n) in enumerate(rec["schedule"]):
            ls = per_gen[g]
            assert sum(L.chunk for L in ls) == int(n), (tag, g)
            assert [L.restart for L in ls] == [1] + [0] * (len(ls) - 1), (tag, g)
            assert all((L.frame, L.is_aux) == (int(fi), int(ia)) and 1 <= L.chunk <= 127 for L in ls), (tag, g)
        assert sum(L.chunk for L in launches) == len(rec["ops"]), tag
        assert [L.pos for L in launches] == np.cumsum([0] + [L.chunk for L in launches[:-1]]).tolist()
    e = FH.expected(tag, rec)[0]
    bad = np.nonzero((e.ops != rec["ops"]).any(axis=1))[0]
    assert len(bad) == 0, "%s: the chunked oracle leaves the recording at opcode %d" % (tag, bad[0])
    assert len(FH.batch(rec)) == FH.N_STREAMS[int(rec["meta"][0])] and len(set(FH.batch(rec))) == len(FH.batch(rec))


@pytest.mark.parametrize("tag", FH.BASE_CASES)
def test_every_pair_hands_over_in_every_phase(corpus, tag):
    """Every generator longer than 2000 opcodes: each ordered pair of forms is a hand-over in each quarter of its real
    opcodes, at least once with both sides in the padding, and one launch begins with real opcodes and ends in padding."""
    rec = corpus[tag]
    forms = FH.forms_of(rec)
    all_pairs = {(a, b) for a in forms for b in forms}
    long_gens = 0
    for which, launches in enumerate(_plans(rec)):
        hand = FH.handovers(launches)
        for g, (fi, ia, start, n, real) in enumerate(FH.segments(rec)):
            if n <= 2000:
                continue
            long_gens += 1
            assert real >= 2000 and n - real >= 2, (tag, g)
            mine = [(pos - start, a, b) for (i, pos, a, b) in hand if launches[i].gen == g]
            counts = []
            for q in range(4):
                lo, hi = real * q // 4, real * (q + 1) // 4
                seen = collections.Counter((a, b) for (p, a, b) in mine if lo <= p < hi)
                assert set(seen) == all_pairs, "%s generator %d quarter %d: no hand-over %s" % (tag, g, q, sorted(all_pairs - set(seen)))
                counts.append(min(seen.values()))
            padded = collections.Counter((a, b) for (p, a, b) in mine if p >= real + 1)     # opcodes p - 1 and p are padding
            assert set(padded) == all_pairs, "%s generator %d: no hand-over in the padding for %s" % (tag, g, sorted(all_pairs - set(padded)))
            across = [L for L in launches if L.gen == g and L.pos - start < real < L.pos - start + L.chunk]
            assert len(across) == 1, (tag, g)
            print("%-32s plan %d generator %d: %4d real + %3d padding, hand-overs per pair and quarter >= %s, in the padding >= %d, "
                  "launch %d-%d crosses the edge under %s" % (tag, which, g, real, n - real, counts, min(padded.values()),
                                                             across[0].pos - start, across[0].pos - start + across[0].chunk, across[0].form))
    assert long_gens >= 2, tag


def test_every_form_creates_a_generator(corpus):
    """every base case has a generator created (restart = 1) by each of its forms, over the plans test_the_matrix runs of it"""
    for tag in FH.BASE_CASES:
        rec = corpus[tag]
        made = [[L.form for L in launches if L.restart] for launches in _plans(rec)]
        print("%-32s generators created under %s" % (tag, made))
        assert {f for m in made for f in m} == set(FH.forms_of(rec)), tag


def test_handovers_meet_the_mt_block_edges(corpus):
    """p = random's draws % 624 at a hand-over, every stream of every case: each receiving form takes over at least once with
    1 .. 8 words left in the block (the block runs out inside its first steps) and once with the block exactly used up
    (p == 0 behind at least one draw: the form that wrote the state left a block of which nothing remains)."""
    near, empty = collections.Counter(), collections.Counter()
    for tag in FH.BASE_CASES:
        rec = corpus[tag]
        streams = FH.expected(tag, rec)
        for launches in _plans(rec):
            for (i, pos, a, b) in FH.handovers(launches):
                for e in streams:
                    d = e.draws_at(pos)
                    p = d % 624
                    if 1 <= 624 - p <= 8:
                        near[b] += 1
                    if p == 0 and d > 0:
                        empty[b] += 1
    print("hand-overs with 1 .. 8 words left, by receiving form: %s; with the block used up: %s" % (dict(near), dict(empty)))
    for f in FH.FORMS:
        assert near[f] >= 1, f
        assert empty[f] >= 1, f
    assert FH.MT_EDGE_HITS == {"near": dict(near), "empty": dict(empty)}       # the numbers DESIGN.md 20 prints
