"""CPU: the oracle against the reference corpus (tests/golden/g11_*.npz, recorded from the imported reference by
tests/golden/make_golden.py --corpus-only on the cases of tests/reference_corpus.py), and the conditions that show the corpus
reaches what it was recorded for: steps decided by the nonces on picture-like content, and the way from the list through
the bag to out-of-work and padding on converging content.  The same recordings are what test_gpu_reference_corpus.py holds
every kernel form to, with no oracle in between."""
import ctypes as C

import numpy as np
import pytest

import reference_corpus as RC


@pytest.fixture(scope="module")
def corpus(golden):
    return RC.load(golden)


def _oracle_run(O, oracle_tables, rec, structured=False, fourth=None, seed_np=None):
    """the oracle on a recording's inputs: (Video, opcodes per segment)"""
    mode, pal, sp, sn, rec_fourth, _ = (int(x) for x in rec["meta"])
    v = O.Video(mode, oracle_tables.get(mode, pal), seed_py=sp, seed_np=sn if seed_np is None else seed_np)
    v.set_fourth_offset(bool(rec_fourth) if fourth is None else fourth)
    frames, out = rec["frames"], []
    for fi, ia, n in rec["schedule"]:
        v.encode_frame(frames[fi, 0], frames[fi, 1] if mode == 1 else None, ia)
        out.append(v.next(int(n), structured=structured))
    return v, out


def _first_difference(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return int(bad[0]) if len(bad) else None


def test_the_corpus_is_complete(corpus):
    """every case of reference_corpus.cases() is recorded, and the corpus has the size and the kinds it was asked to have"""
    cases = RC.cases()
    assert sorted(c.tag for c in cases) == sorted(corpus)
    assert len(cases) >= 20
    total = sum(len(r["ops"]) for r in corpus.values())
    longest = max(len(r["ops"]) for r in corpus.values())
    print("%d recordings, %d opcodes, longest %d" % (len(corpus), total, longest))
    assert total >= 25000 and longest <= RC.MAX_OPS
    for kind in ("img", "static", "dither", "flat"):
        seen = {(c.mode, c.palette) for c in cases if c.kind == kind}
        assert {m for m, _ in seen} == {RC.HGR, RC.DHGR}, kind
        assert RC.IIGS in {p for _, p in seen}, kind
    assert len({RC.img_parameters(s)[:2] for s in (101, 102, 103, 104)}) >= 2       # periods and speeds of the img cases
    fourth = [c for c in cases if c.fourth]
    assert sorted((c.mode, c.kind) for c in fourth) == [(0, "img"), (0, "static"), (1, "img"), (1, "static")]
    for c in cases:
        rec = corpus[c.tag]
        assert rec["meta"].tolist() == c.meta().tolist(), c.tag
        assert int(rec["schedule"][:, 2].sum()) == len(rec["ops"]), c.tag


@pytest.mark.parametrize("structured", [False, True])
def test_oracle_reproduces_the_corpus(O, oracle_tables, corpus, structured):
    """opcodes, both memory maps, both priority arrays, the packed screen, out_of_work and the next four draws of both RNG
    streams, for the literal heap form and for the restructured form the kernels implement -- the comparison
    test_oracle_golden.py makes for g3.  The fourth-offset recordings run with set_fourth_offset(True)."""
    L = O.lib()
    for tag in sorted(corpus):
        rec = corpus[tag]
        mode = int(rec["meta"][0])
        v, out = _oracle_run(O, oracle_tables, rec, structured=structured)
        out = np.concatenate(out)
        bad = _first_difference(out, rec["ops"])
        assert bad is None, "%s: first difference at opcode %d: oracle %s, reference %s" % (tag, bad, out[bad], rec["ops"][bad])
        assert (v.memory(0) == rec["mem_main"]).all(), tag
        assert (v.update_priority(0) == rec["up_main"]).all(), tag
        assert (v.packed == rec["packed"]).all(), tag
        if mode == 1:
            assert (v.memory(1) == rec["mem_aux"]).all(), tag
            assert (v.update_priority(1) == rec["up_aux"]).all(), tag
        assert [int(v.out_of_work(0)), int(v.out_of_work(1))] == rec["out_of_work"].tolist(), tag
        rp, rn = v.rng_py(), v.rng_np()
        assert [L.orc_py_getrandbits8(C.byref(rp)) for _ in range(4)] == rec["py_next"].tolist(), tag
        assert [L.orc_np_randint256(C.byref(rn)) for _ in range(4)] == rec["np_next"].tolist(), tag


def test_fourth_offset_changes_the_stream(O, oracle_tables, corpus):
    """the four recordings made with the reference's exit test at 4 differ from the recordings of the same inputs without it,
    and so does the oracle without the flag"""
    tags = [t for t in sorted(corpus) if int(corpus[t]["meta"][4])]
    assert len(tags) == 4
    for tag in tags:
        rec, base = corpus[tag], corpus[tag[:-len("_fourth")]]
        assert (rec["frames"] == base["frames"]).all() and (rec["schedule"] == base["schedule"]).all(), tag
        assert rec["meta"][:4].tolist() == base["meta"][:4].tolist() and not int(base["meta"][4]), tag
        assert (rec["ops"] != base["ops"]).any(), tag
        assert (rec["ops"][:, 5] != rec["ops"][:, 2]).any(), tag          # a real fourth offset, not the copy of the first
        _, out = _oracle_run(O, oracle_tables, rec, fourth=False)
        assert (np.concatenate(out) != rec["ops"]).any(), tag
        assert (np.concatenate(out) == base["ops"]).all(), tag


def test_nonces_decide_steps_on_picture_like_content(O, oracle_tables, corpus):
    """img, dither, flat: the oracle under seed_np + 1 -- other nonces, everything else the same -- leaves the recorded stream
    within the case's length, so at least one recorded step was decided by a nonce.  Prints where."""
    for c in RC.cases():
        if c.kind not in RC.TIE_KINDS:
            continue
        rec = corpus[c.tag]
        _, out = _oracle_run(O, oracle_tables, rec, seed_np=c.seed_np + 1)
        bad = _first_difference(np.concatenate(out), rec["ops"])
        print("%-28s %5d opcodes, another np seed diverges at opcode %s" % (c.tag, len(rec["ops"]), bad))
        assert bad is not None, "%s: no step of this case is decided by a nonce" % c.tag


def _segments(rec):
    pos = 0
    for fi, ia, n in rec["schedule"]:
        yield int(fi), int(ia), rec["ops"][pos:pos + int(n)]
        pos += int(n)


def _trailing_padding(rec, fi, ia, ops):
    pad = RC.is_padding(ops, rec["frames"], fi, ia)
    real = np.nonzero(~pad)[0]
    return len(ops) - (int(real.max()) + 1 if len(real) else 0)


def test_exhaustion_cases_reach_padding(corpus):
    """both out_of_work flags that the schedule touches are set in the recording, and the recording ends in padding"""
    seen = 0
    for c in RC.cases():
        if not c.exhaust:
            continue
        seen += 1
        rec = corpus[c.tag]
        for bank in sorted(set(int(a) for a in rec["schedule"][:, 1])):
            assert rec["out_of_work"][bank] == 1, (c.tag, bank)
        fi, ia, ops = list(_segments(rec))[-1]
        assert _trailing_padding(rec, fi, ia, ops) >= 2, c.tag
    assert seen >= 4 + 2      # img and static in both modes, and the two static ones again with the fourth offset


def test_static_cases_run_out_of_work(O, oracle_tables, corpus):
    """static: at least one generator gave fewer real opcodes than were pulled from it -- the rest is padding, and it is the
    segment in which the (oracle's) out_of_work flag of its bank comes up"""
    for c in RC.cases():
        if c.kind != "static":
            continue
        rec = corpus[c.tag]
        short = [(k, len(ops), _trailing_padding(rec, fi, ia, ops)) for k, (fi, ia, ops) in enumerate(_segments(rec))]
        short = [s for s in short if s[2] >= 2]
        print("%-32s generators that ran dry (index, pulled, padding): %s" % (c.tag, short))
        assert short, c.tag
        mode = int(rec["meta"][0])
        ov = O.Video(mode, oracle_tables.get(mode, c.palette), seed_py=c.seed_py, seed_np=c.seed_np)
        ov.set_fourth_offset(c.fourth)
        for k, (fi, ia, n) in enumerate(rec["schedule"]):
            ov.encode_frame(rec["frames"][fi, 0], rec["frames"][fi, 1] if mode == 1 else None, ia)
            ov.next(int(n))
            if k == short[0][0]:
                assert ov.out_of_work(ia), c.tag
                break
            assert not ov.out_of_work(ia), c.tag


def test_stored_frames_are_legal_targets(corpus):
    """no byte in a screen hole and, in DHGR, no bit 7 (the reference asserts on those: g10 covers that side); the HGR cases
    of the kinds that can have both palette bits in one screen have them"""
    kinds = {c.tag: c.kind for c in RC.cases()}
    for tag, rec in sorted(corpus.items()):
        frames, mode = rec["frames"], int(rec["meta"][0])
        assert frames.dtype == np.uint8 and frames.shape[1:] == (2 if mode == 1 else 1, 32, 256), tag
        assert not frames[..., RC.HOLES].any(), tag
        if mode == 1:
            assert not (frames & 0x80).any(), tag
        elif kinds[tag] in ("dither", "static", "flat"):
            visible = frames[:, 0][..., ~RC.HOLES]
            both = ((visible & 0x80) != 0).any(axis=(1, 2)) & ((visible & 0x80) == 0).any(axis=(1, 2))
            assert both.any(), "%s: no HGR screen with bit 7 both set and clear" % tag


def test_builders_rebuild_the_stored_frames(corpus):
    """A note about the builders of reference_corpus.py, NOT about the recordings: on this numpy / torch they still make the
    frames that were recorded.  The fixture stores the frames, and every other test reads them from there; if this fails
    (it names the cases), a generator changed -- that is no reason to record again."""
    moved = [c.tag for c in RC.cases() if not np.array_equal(c.frames(), corpus[c.tag]["frames"])]
    assert not moved, "builders no longer make the stored frames of: %s" % ", ".join(moved)
