"""GPU: SURVEY 8(f4) -- joint choice of the content byte, the "global optimization" the reference's
README.md:212-215 leaves as future work.  There is NO reference behaviour to match: the definition
is oracle/iiv_oracle.c:choose_content_joint (= include/iivision.h IIV_CONTENT_JOINT); these tests
hold the kernel to that definition bit for bit and check what the mode is for -- less error left on
the screen for the same number of opcodes -- and that the default stays the reference's greedy step."""

import numpy as np
import pytest

import encode_harness as H

pytestmark = pytest.mark.gpu


def _device(native, device_tables, mode, frames_list, sched, seeds, O, joint, fourth=False):
    enc = H.make_encoder(native, device_tables, mode, n_streams=len(frames_list), fourth=fourth, joint=joint, rng=seeds, O=O)
    fm, fa = H.device_frames(mode, frames_list)
    ops = enc.encode(fm, fa, H.segments(sched))
    enc.check()
    return enc, ops.cpu().numpy()


def _oracle(O, oracle_tables, mode, frames, sched, sp, sn, joint, fourth=False):
    return H.oracle_run(O, oracle_tables, mode, 5, frames, sched, (sp, sn), fourth=fourth, joint=joint)


@pytest.mark.parametrize("fourth", [False, True])
@pytest.mark.parametrize("impl", [True, "split"])
@pytest.mark.parametrize("mode", [1, 0])
def test_joint_steps_equal_the_definition(native, O, oracle_tables, device_tables, mode, impl, fourth):
    """Four streams (iid and coherent data), generators on both banks, a continued frame: opcodes,
    memory maps, priorities (the primary keeps its residual), packed screen and both RNG positions
    equal the oracle's joint run -- both implementations (packed 16-bit sums of the narrow form, IIV_CONTENT_JOINT;
    the two-component split table one byte value at a time, IIV_CONTENT_JOINT_SPLIT), and (round 6) both together with
    the fourth offset per opcode (IIV_OPT_FOURTH_OFFSET: the joint score then takes three deltas)."""
    n = 4
    sched = [(0, 0, 60), (0, 1 if mode == 1 else 0, 45), (1, 0, 70), (1, 1 if mode == 1 else 0, 1), (2, 0, 40)]
    frames = [H.synth(mode, 3, 300 + i, coherent=(i % 2 == 1)) for i in range(n)]
    seeds = [(i + 5, 70 + i) for i in range(n)]
    enc, got = _device(native, device_tables, mode, frames, sched, seeds, O, impl, fourth)
    differs_from_greedy = 0
    if fourth:   # (the mode does hand out a fourth offset)
        o = np.sort(got[0][:, 2:6], axis=1)
        assert ((o[:, 1:] != o[:, :-1]).sum(axis=1) + 1).max() == 4
    for i in range(n):
        v, exp = _oracle(O, oracle_tables, mode, frames[i], sched, *seeds[i], True, fourth)
        H.check_ops(got[i], exp, "stream %d" % i)
        H.check_oracle_state(native, enc, i, v, mode, "stream %d" % i)
        _, greedy = _oracle(O, oracle_tables, mode, frames[i], sched, *seeds[i], False, fourth)
        differs_from_greedy += int((greedy != exp).any())
    enc.close()
    assert differs_from_greedy == n          # the mode really does something else


@pytest.mark.parametrize("mode", [1, 0])
def test_joint_leaves_less_error_per_opcode(native, O, device_tables, mode):
    """What the mode is for: the same clips and opcode budget (three Movie-paced frames), less
    perceptual error left between screen and target.  R(target byte) <= R(chosen byte) holds step by
    step only in the step's own accounting (stores are scored against the target's neighbours,
    screen.py:542-545), and the two trajectories differ, so the claim is checked on the outcome:
    every one of 8 clips ends with less error, 2-6 % less in total."""
    n = 8
    sched = ([(0, 0, 292), (0, 1, 198), (1, 1, 94), (1, 0, 292), (1, 1, 104), (2, 1, 188), (2, 0, 292), (2, 1, 10)]
             if mode == 1 else [(0, 0, 490), (1, 0, 490), (2, 0, 490)])
    frames = [H.synth(mode, 3, 900 + i, coherent=(i % 2 == 1)) for i in range(n)]
    seeds = [(i + 1, i + 1) for i in range(n)]
    res = {}
    for joint in (False, True):
        enc, ops = _device(native, device_tables, mode, frames, sched, seeds, O, joint)
        res[joint] = H.screen_error(native, device_tables, mode, enc, frames, 2, n)
        enc.close()
    assert (res[True] < res[False]).all(), (res[True], res[False])
    gain = 1.0 - res[True].sum() / res[False].sum()
    assert 0.01 < gain < 0.2, gain


@pytest.mark.parametrize("mode,ops,impl,fourth", [(1, 6000, True, False), (0, 4500, True, False), (1, 6000, "split", False), (1, 5000, True, True), (0, 4000, "split", True)])
def test_joint_runs_past_the_list_into_the_bag(native, O, oracle_tables, device_tables, mode, ops, impl, fourth):
    """A generator pulled far past its sorted list: the joint choice leaves a primary with a residual priority (it is not
    re-queued, video.py:140 with IIV_CONTENT_JOINT), so a stale bag entry of that location, pushed when it was an extra
    offset, finds it live when it is popped and the location is encoded again -- as the oracle's definition does.  (Until
    round 3 the kernel dropped such pops: every joint test stopped short of the bag.)"""
    import stream_batch
    n = 2
    fm, fa = stream_batch.synth_frames_torch(n, 2, mode == 1, seed=5, coherent=True, device="cpu", keep=0.97)
    frames = [np.stack([fm[i].numpy(), fa[i].numpy() if fa is not None else np.zeros_like(fm[i].numpy())], axis=1) for i in range(n)]
    sched = [(0, 0, ops), (1, 0, 1500)]
    seeds = [(i + 3, i + 9) for i in range(n)]
    enc, got = _device(native, device_tables, mode, frames, sched, seeds, O, impl, fourth)
    for i in range(n):
        v, exp = _oracle(O, oracle_tables, mode, frames[i], sched, *seeds[i], True, fourth)
        H.check_ops(got[i], exp, "stream %d" % i)
        H.check_oracle_state(native, enc, i, v, mode, "stream %d" % i)
    enc.close()


def test_default_is_the_reference_step(native, O, oracle_tables, device_tables):
    """The flag is off unless asked for, and switching it off again restores the reference's stream."""
    mode = 1
    frames = [H.synth(mode, 1, 41)]
    sched = [(0, 0, 80)]
    enc, a = _device(native, device_tables, mode, frames, sched, [(2, 3)], O, False)
    enc.close()
    _, exp = _oracle(O, oracle_tables, mode, frames[0], sched, 2, 3, False)
    assert (a[0] == exp).all()
    enc = H.make_encoder(native, device_tables, mode, joint=True, rng=[(2, 3)], O=O)
    enc.set_content_choice(False)      # (switched off again: the call under test)
    fm, fa = H.device_frames(mode, frames)
    assert (enc.encode(fm, fa, [(0, 0, 1, 80)]).cpu().numpy()[0] == exp).all()
    enc.close()


def test_dropin_video_joint_content(O, oracle_tables):
    """The Python mirror's Video(joint_content=True): the lazy generator -- speculative chunks,
    abandoned generators, a mid-stream state read -- yields the oracle's joint stream, and the
    global random / np.random generators end where that run's end."""
    import contextlib
    import io
    import random
    import palette
    import screen
    import video
    import video_mode

    class FG:
        input_frame_rate = 30

    mode = 1
    frames = H.synth(mode, 2, 4242)
    sched = [(0, 0, 70), (0, 1, 30), (1, 1, 25)]
    random.seed(9)
    np.random.seed(11)
    v = video.Video(FG(), ticks_per_second=14700., mode=video_mode.VideoMode.DHGR, palette=palette.Palette.NTSC,
                    joint_content=True)
    v.SPECULATE = 16
    got = []
    with contextlib.redirect_stdout(io.StringIO()):
        for fi, ia, n in sched:
            tgt = screen.DHGRBitmap(main_memory=screen.MemoryMap(1, frames[fi, 0].copy()),
                                    aux_memory=screen.MemoryMap(1, frames[fi, 1].copy()), palette=palette.Palette.NTSC)
            gen = v.encode_frame(tgt, is_aux=bool(ia))
            for k in range(n):
                page, content, offsets = next(gen)
                got.append([page, content] + list(offsets))
                if k == 20:
                    mm = v.aux_memory_map if ia else v.memory_map
                    assert mm.page_offset[page - 32, offsets[0]] == content
    ov, exp = _oracle(O, oracle_tables, mode, frames, sched, 9, 11, True)
    assert (np.array(got, dtype=np.uint8) == exp).all()
    assert (v.memory_map.page_offset == ov.memory(0)).all() and (v.aux_memory_map.page_offset == ov.memory(1)).all()
    assert (v.update_priority == ov.update_priority(0)).all() and (v.aux_update_priority == ov.update_priority(1)).all()
    py, npd = ov.rng_py(), ov.rng_np()
    L = O.lib()
    import ctypes as C
    assert [random.getrandbits(8) for _ in range(4)] == [L.orc_py_getrandbits8(C.byref(py)) for _ in range(4)]
    assert np.random.randint(0, 256, size=4).tolist() == [L.orc_np_randint256(C.byref(npd)) for _ in range(4)]


def test_options_that_need_the_diff_matrix_say_so(native, device_tables):
    """An encoder made without dm (caller's own tables) has no split tables: the joint content choice,
    the split diff-weight mode and the one-wave / team kernels refuse instead of reading nothing."""
    enc = H.make_encoder(native, device_tables, 1, dm=False)
    for call in (lambda: enc.set_content_choice(True), lambda: enc.set_diff_weights_mode("split"),
                 lambda: enc.set_greedy_kernel(True), lambda: enc.set_greedy_kernel("team")):
        with pytest.raises(native.IIVError):
            call()
    enc.set_content_choice(False)      # (the defaults stay available)
    enc.set_diff_weights_mode("table")
    enc.close()
    with pytest.raises(native.IIVError):
        native.check(native.lib().iiv_build_narrow_store_table(1, None, None, None, None, None))
