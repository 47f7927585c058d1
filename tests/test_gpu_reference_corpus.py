"""GPU: every kernel form against the reference corpus (tests/golden/g11_*.npz; tests/reference_corpus.py says what is in
it) -- the reference's own opcodes, state and RNG positions on picture-like content, where the nonces decide most steps, and
on converging content, through the bag to out-of-work and padding.  No oracle stands between the kernels and the
recordings here; test_reference_corpus.py holds the oracle to the same files on the CPU."""
import contextlib
import io
import random

import numpy as np
import pytest

import encode_harness as H
import reference_corpus as RC

pytestmark = pytest.mark.gpu

FORMS = [(True, True), (False, True), (True, False), (False, False), (True, "team"), ("split", True), ("split", "team"),
         ("split", False), (True, "shared"), (False, "shared")]      # (diff weights, greedy kernel): test_golden_runs' ten


@pytest.fixture(scope="module")
def corpus(golden):
    return RC.load(golden)


def _meta(rec):
    mode, pal, sp, sn, fourth, _ = (int(x) for x in rec["meta"])
    return mode, pal, sp, sn, bool(fourth)


def _check_stream(native, O, enc, i, got, rec, what):
    H.check_ops(got, rec["ops"], what)
    H.check_recorded_state(native, O, enc, i, rec, what)


def _one_stream(native, O, device_tables, rec, tag, recurrence, kernel, prefix):
    mode, pal, sp, sn, fourth = _meta(rec)
    enc = H.make_encoder(native, device_tables, mode, pal, dw=recurrence, kernel=kernel, prefix=prefix, rng=[(sp, sn)], O=O,
                         **({"fourth": True} if fourth else {}))
    fm, fa = H.device_frames(mode, [rec["frames"]])
    got = enc.encode(fm, fa, H.segments(rec["schedule"]))
    enc.check()
    _check_stream(native, O, enc, 0, got.cpu().numpy()[0], rec, "%s (prefix sort %s)" % (tag, "on" if prefix else "off"))
    enc.close()


@pytest.mark.parametrize("recurrence,wave", FORMS)
def test_every_form_reproduces_the_corpus(native, O, corpus, device_tables, recurrence, wave):
    """Every recording made without the fourth offset (that option runs in three kernels: test_fourth_offset_corpus), as a
    one-stream encoder, in each (diff-weights mode, greedy kernel) pair of test_golden_runs, with the prefix sort on and
    off: opcodes, both memory maps, both priority arrays, the packed screen, out_of_work and the next draws of both RNG
    streams are the reference's."""
    tags = [t for t in sorted(corpus) if not _meta(corpus[t])[4]]
    assert len(tags) >= 20
    for tag in tags:
        for prefix in (True, False):
            _one_stream(native, O, device_tables, corpus[tag], tag, recurrence, wave, prefix)


@pytest.mark.parametrize("kernel", ["plain", "shared", "team"])
@pytest.mark.parametrize("prefix", [True, False])
def test_fourth_offset_corpus(native, O, corpus, device_tables, kernel, prefix):
    """the four recordings made with the reference's exit test reading 4, with set_fourth_offset(True), in the kernels that
    have the option: the two one-wave forms and the eight-wave team kernel"""
    tags = [t for t in sorted(corpus) if _meta(corpus[t])[4]]
    assert len(tags) == 4
    for tag in tags:
        _one_stream(native, O, device_tables, corpus[tag], tag, True, kernel, prefix)


GROUPS = [(RC.HGR, RC.NTSC), (RC.HGR, RC.IIGS), (RC.DHGR, RC.NTSC), (RC.DHGR, RC.IIGS)]


@pytest.mark.parametrize("mode,pal", GROUPS)
@pytest.mark.parametrize("kernel", ["shared", "plain"])
def test_corpus_as_one_batch(native, O, corpus, device_tables, mode, pal, kernel):
    """All cases of a (mode, palette) as the streams of one encoder, each with its own schedule (encode_streams), in the
    corpus' order and reversed: tie-heavy and tie-free streams, one-opcode generators and runs into padding share the
    launches -- and, under "shared", the workgroups, which take them off the queue in both orders.  In DHGR the streams of a
    round sit on different banks, which the shared form cannot serve: those launches fall back to the plain form
    (test_encode_streams_whose_rounds_mix_banks_run_the_plain_form).  Every stream equals its recording either way."""
    tags = [t for t in sorted(corpus) if _meta(corpus[t])[:2] == (mode, pal) and not _meta(corpus[t])[4]]
    assert len(tags) >= 3, tags
    for order in (tags, tags[::-1]):
        recs = [corpus[t] for t in order]
        enc = H.make_encoder(native, device_tables, mode, pal, len(recs), dw=True, kernel=kernel, prefix=True,
                             rng=[_meta(r)[2:4] for r in recs], O=O)
        fm, fa = H.device_frames(mode, [r["frames"] for r in recs])
        enc.profile(True)
        ops, totals = enc.encode_streams(fm, fa, [H.segments(r["schedule"]) for r in recs])
        enc.check()
        print("%s pal %d, kernel=%r: greedy launches by form %s" % ("DHGR" if mode else "HGR", pal, kernel, enc.launch_forms()))
        got = ops.cpu().numpy()
        for i, (tag, rec) in enumerate(zip(order, recs)):
            assert totals[i] == len(rec["ops"]), tag
            _check_stream(native, O, enc, i, got[i, :totals[i]], rec, "%s as stream %d of %d" % (tag, i, len(order)))
            assert not got[i, totals[i]:].any(), "%s: opcodes written behind the stream's own" % tag
        enc.close()


class _FG:
    input_frame_rate = 30


def _video_run(rec, speculate, ticked):
    """the drop-in transcoder/video.Video on a recording's inputs, pulled as the recording was (one generator per schedule
    entry, abandoned after its opcodes); ticked: tick() before every opcode as movie.py does, which is what lets the Video
    size its launches and enqueue the generator behind a bank flip ahead of the caller"""
    import palette
    import screen
    import video
    import video_mode
    mode, pal, sp, sn, _ = _meta(rec)
    frames = rec["frames"]
    random.seed(sp)
    np.random.seed(sn)
    v = video.Video(_FG(), ticks_per_second=14700., mode=video_mode.VideoMode.DHGR if mode else video_mode.VideoMode.HGR,
                    palette=palette.Palette(pal))
    v.SPECULATE = speculate
    got, ticks, last_frame = [], 0, -1
    with contextlib.redirect_stdout(io.StringIO()):
        for fi, ia, n in rec["schedule"]:
            gen = None
            for k in range(int(n)):
                if ticked:
                    ticks += 1
                    new_frame = v.tick(ticks)
                    assert bool(new_frame) == (k == 0 and fi != last_frame), (fi, ia, k, ticks)
                if gen is None:
                    main = screen.MemoryMap(1, frames[fi, 0].copy())
                    if mode == 1:
                        tgt = screen.DHGRBitmap(main_memory=main, aux_memory=screen.MemoryMap(1, frames[fi, 1].copy()), palette=palette.Palette(pal))
                    else:
                        tgt = screen.HGRBitmap(main_memory=main, palette=palette.Palette(pal))
                    gen = v.encode_frame(tgt, is_aux=bool(ia))
                page, content, offsets = next(gen)
                got.append([page, content] + list(offsets))
            last_frame = fi
    got = np.array(got, dtype=np.uint8)
    bad = np.nonzero((got != rec["ops"]).any(axis=1))[0]
    assert len(bad) == 0, "first mismatch at op %d: got %s want %s" % (bad[0], got[bad[0]], rec["ops"][bad[0]])
    assert (v.memory_map.page_offset == rec["mem_main"]).all()
    assert (v.update_priority == rec["up_main"]).all()
    assert (v.pixelmap.packed == rec["packed"]).all()
    if mode == 1:
        assert (v.aux_memory_map.page_offset == rec["mem_aux"]).all()
        assert (v.aux_update_priority == rec["up_aux"]).all()
    assert [int(v.out_of_work[False]), int(v.out_of_work[True])] == rec["out_of_work"].tolist()
    assert [random.getrandbits(8) for _ in range(4)] == rec["py_next"].tolist()
    assert np.random.randint(0, 256, size=4).tolist() == rec["np_next"].tolist()
    return v


@pytest.mark.parametrize("tag", ["HGR_img_movie", "DHGR_img_movie"])
def test_dropin_video_on_picture_like_content(corpus, tag):
    """One Movie-paced img case per mode through transcoder/video.Video, as test_gpu_dropin.py drives a g3 tag, against the
    recording.  Paced as movie.py paces it (tick() per opcode, SPECULATE None): launches sized to what is pulled, handed out
    live while the kernel runs, in DHGR the generator behind each bank flip inside a frame enqueued ahead and adopted.  Then
    in speculative chunks of 48 without the pacing: every generator is abandoned inside a chunk, rolled back and replayed."""
    rec = corpus[tag]
    v = _video_run(rec, None, True)
    assert v.LIVE and v.live_stats["launches"] >= 1
    st = v.lookahead_stats
    print(tag, "live", v.live_stats, "look-ahead", st)
    if _meta(rec)[0] == 1:
        # every generator behind a bank flip inside a frame was enqueued ahead, was the one then asked for, none was undone
        # (what test_movie_paced_generators_are_single_launches finds on noise)
        flips = sum(1 for j in range(1, len(rec["schedule"])) if rec["schedule"][j][0] == rec["schedule"][j - 1][0])
        assert flips >= 3 and st["launched"] == st["adopted"] == flips and st["undone"] == 0, (st, flips)
    else:
        assert st["launched"] == 0, st
    _video_run(rec, 48, False)
