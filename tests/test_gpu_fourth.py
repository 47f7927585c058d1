"""GPU: SURVEY 8(f4) -- a real fourth offset per opcode (IIV_OPT_FOURTH_OFFSET).  The player stores every opcode's
content byte at four offsets and video.py:146 says "Need to find 3 more offsets to fill this opcode", but the loop's exit
test `len(offsets) == 3` (video.py:180-181) counts the primary, so the reference finds two and repeats the first
(:184-186).  With the option the test reads 4.  NOT the reference's stream -- but it IS the reference's loop with one
literal changed, and that is what pins it: tests/golden/g8_fourth_offset.npz holds runs of the imported reference with
exactly that change (make_golden.py --fourth-only); the oracle equals them on the CPU (test_oracle_golden.py), and these
tests hold the kernel to both."""

import numpy as np
import pytest

import encode_harness as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("recurrence,prefix,kernel", [(True, True, None), (False, False, "team"), ("split", True, False), (True, False, "shared")])
def test_reference_with_exit_test_at_four(native, O, golden, device_tables, recurrence, prefix, kernel):
    """The reference's own runs with `len(offsets) == 4`: opcodes, memory maps, priorities, packed screen,
    out_of_work and both RNG positions, incl. runs to exhaustion (bag phase with three pushes per step, padding)."""
    g8 = golden.g8_fourth_offset
    for tag in H.tags(g8):
        rec = H.recorded(g8, tag)
        mode, pal, sp, sn = (int(x) for x in rec["meta"])
        # (the option runs in the one-wave and the eight-wave kernel; others fall back to the one-wave)
        enc = H.make_encoder(native, device_tables, mode, pal, dw=recurrence, kernel=kernel, prefix=prefix, fourth=True,
                             rng=[(sp, sn)], O=O)
        fm, fa = H.device_frames(mode, [rec["frames"]])
        got = enc.encode(fm, fa, H.segments(rec["schedule"])).cpu().numpy()
        enc.check()
        H.check_ops(got[0], rec["ops"], tag)
        H.check_recorded_state(native, O, enc, 0, rec, tag)
        enc.close()


@pytest.mark.parametrize("mode,kind", [(1, "iid"), (0, "iid"), (1, "img"), (0, "img"), (1, "static"), (0, "coh")])
def test_movie_paced_batches_equal_the_oracle(native, O, oracle_tables, device_tables, mode, kind):
    """Sixteen clips per input kind through the Movie-paced batch driver (bank flips, continued generators, prefix
    selection with 4 entries per opcode): every stream equals the oracle run with the same flag.  Picture-like input
    ties on nearly every step (three winners out of ~11 equal deltas), converging input ends in the bag."""
    import stream_batch
    n, nf = 16, 6
    if kind == "img":
        fm, fa = stream_batch.synth_frames_img(n, nf, mode == 1, seed=77, device="cpu")
    else:
        fm, fa = stream_batch.synth_frames_torch(n, nf, mode == 1, seed=78, coherent=kind != "iid", device="cpu",
                                                 keep=0.98 if kind == "static" else 0.9, repeat=2 if kind == "static" else 1)
    t, s = device_tables.get(mode, 5)
    seeds = [(100 + i, 200 + i) for i in range(n)]
    b = stream_batch.StreamBatch(mode, t, s, n, seeds=seeds, dm=device_tables.dm[(mode, 5)], fourth_offset=True)
    ops, segs = b.encode_frames(fm.cuda(), fa.cuda() if fa is not None else None, nf)
    b.enc.check()
    got = ops.cpu().numpy()
    four = 0
    for i in range(n):
        frames = np.stack([fm[i].numpy(), (fa if fa is not None else fm)[i].numpy()], axis=1)      # (HGR: bank 1 is not read)
        v, exp = H.oracle_run(O, oracle_tables, mode, 5, frames, segs, seeds[i], fourth=True)
        H.check_ops(got[i], exp, "stream %d" % i)
        H.check_oracle_state(native, b.enc, i, v, mode, "stream %d" % i)
        four += int((exp[:, 5] != exp[:, 2]).sum())
    b.close()
    assert four > 0     # fourth offsets that are not a copy of the first


@pytest.mark.parametrize("mode", [1, 0])
def test_fourth_offset_leaves_less_error_per_opcode(native, O, device_tables, mode):
    """What the option is for: the same clips, the same opcode budget (three Movie-paced frames), a third more useful
    stores -- every one of 8 clips ends with less perceptual error between screen and target."""
    n = 8
    sched = ([(0, 0, 292), (0, 1, 198), (1, 1, 94), (1, 0, 292), (1, 1, 104), (2, 1, 188), (2, 0, 292), (2, 1, 10)]
             if mode == 1 else [(0, 0, 490), (1, 0, 490), (2, 0, 490)])
    frames = [H.synth(mode, 3, 900 + i, coherent=(i % 2 == 1)) for i in range(n)]
    fm, fa = H.device_frames(mode, frames)
    res = {}
    for fourth in (False, True):
        enc = H.make_encoder(native, device_tables, mode, n_streams=n, fourth=fourth, rng=[(i + 1, i + 1) for i in range(n)], O=O)
        enc.encode(fm, fa, H.segments(sched))
        enc.check()
        res[fourth] = H.screen_error(native, device_tables, mode, enc, frames, 2, n)
        enc.close()
    assert (res[True] < res[False]).all(), (res[True], res[False])
    gain = 1.0 - res[True].sum() / res[False].sum()
    assert 0.005 < gain < 0.3, gain


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("fourth", [False, True])
def test_team_kernel_to_exhaustion_on_picture_like_input(native, O, oracle_tables, device_tables, mode, fourth):
    """The eight-wave kernel (one clip alone: what a single video.Video uses), with and without the option, on
    picture-like input (nearly every step is decided by the nonces) through the list, the re-queued bag -- wave 0 alone,
    ties resolved there too -- and out of work: every opcode equals the oracle's."""
    import stream_batch
    n, nf = 4, 2
    fm, fa = stream_batch.synth_frames_img(n, nf, mode == 1, seed=31, device="cpu")
    sched = [(0, 0, 1, 2500), (0, 0, 0, 2500), (1, 0, 1, 3000), (1, 0, 0, 3000)]
    seeds = [(i + 3, i + 9) for i in range(n)]
    enc = H.make_encoder(native, device_tables, mode, n_streams=n, dw=True, kernel="team", prefix=True, fourth=fourth, rng=seeds, O=O)
    got = enc.encode(fm.cuda(), fa.cuda() if fa is not None else None, sched).cpu().numpy()
    enc.check()
    for i in range(n):
        frames = np.stack([fm[i].numpy(), (fa if fa is not None else fm)[i].numpy()], axis=1)      # (HGR: bank 1 is not read)
        v, exp = H.oracle_run(O, oracle_tables, mode, 5, frames, sched, seeds[i], fourth=fourth)
        H.check_ops(got[i], exp, "stream %d" % i)
        assert v.out_of_work(0)
        H.check_oracle_state(native, enc, i, v, mode, "stream %d" % i)
    enc.close()


def test_option_rules(native, device_tables):
    """Off unless asked for; needs the split store table (dm); together with the joint content choice since round 6, in
    either order (tests/test_gpu_joint.py holds the pair to the oracle's definition)."""
    enc = H.make_encoder(native, device_tables, 1)
    enc.set_fourth_offset(True)                # (the order of these calls is what is tested: made here, not by the harness)
    enc.set_content_choice(True)
    enc.set_fourth_offset(False)
    enc.set_content_choice(True)
    enc.set_fourth_offset(True)
    enc.close()
    enc = H.make_encoder(native, device_tables, 1, dm=False)          # no dm: workgroup kernel only
    with pytest.raises(native.IIVError):
        enc.set_fourth_offset(True)
    enc.close()


def test_dropin_video_fourth_offset(O, oracle_tables):
    """The Python mirror's Video(fourth_offset=True): the lazy generator yields the oracle's stream with the flag."""
    import contextlib
    import io
    import random
    import palette
    import screen
    import video
    import video_mode

    class FG:
        input_frame_rate = 30.0

    mode = 1
    frames = H.synth(mode, 2, 51)
    random.seed(4)
    np.random.seed(4)
    v = video.Video(FG(), 14700.0, mode=video_mode.VideoMode.DHGR, palette=palette.Palette.NTSC, fourth_offset=True)
    got = []
    with contextlib.redirect_stdout(io.StringIO()):
        for (fi, ia, k) in [(0, False, 120), (0, True, 77), (1, True, 140)]:
            tgt = screen.DHGRBitmap(palette.Palette.NTSC, screen.MemoryMap(1, frames[fi, 0].copy()), screen.MemoryMap(1, frames[fi, 1].copy()))
            gen = v.encode_frame(tgt, ia)
            for _ in range(k):
                page, content, offs = next(gen)
                got.append([page, content] + list(offs))
    o = O.Video(mode, oracle_tables.get(mode, 5), seed_py=4, seed_np=4)
    o.set_fourth_offset(True)
    exp = []
    for (fi, ia, k) in [(0, 0, 120), (0, 1, 77), (1, 1, 140)]:
        o.encode_frame(frames[fi, 0], frames[fi, 1], ia)
        exp.append(o.next(k))
    assert (np.array(got, np.uint8) == np.concatenate(exp)).all()
    assert (v.update_priority == o.update_priority(0).reshape(32, 256)).all()
