"""GPU: edge cases and size-independent properties of the encode path, checked
against the oracle where it finishes in seconds and through invariants at full
batch size."""

import numpy as np
import pytest

import encode_harness as H

pytestmark = pytest.mark.gpu

HOLES = (np.arange(256) & 127) >= 120


def _encode(native, device_tables, mode, frames, sched, seeds, O, wave=None, prefix=True, init=None):
    """frames: (n_streams, n_frames, 2, 32, 256)."""
    enc = H.make_encoder(native, device_tables, mode, n_streams=frames.shape[0], kernel=wave, prefix=prefix)
    for i, (a, b) in enumerate(seeds):      # (one set_state per stream, on purpose: the other tests upload with set_state_all)
        py, npw = H.seed_states(O, a, b)
        enc.set_state(native.STATE_RNG_PY, py, i)
        enc.set_state(native.STATE_RNG_NP, npw, i)
    if init:
        init(enc)
    fm, fa = H.device_frames(mode, list(frames))
    ops = enc.encode(fm, fa, sched)
    enc.check()
    return enc, ops.cpu().numpy()


def _oracle(O, oracle_tables, mode, frames1, sched, seed, init=None):
    return H.oracle_run(O, oracle_tables, mode, 5, frames1, sched, seed, init=init)


@pytest.mark.parametrize("wave", [True, False, "shared"])
def test_blank_target_on_blank_screen(native, O, device_tables, wave):
    """Nothing to do: no RNG draw, out_of_work at once, only padding opcodes."""
    frames = np.zeros((1, 1, 2, 32, 256), np.uint8)
    enc, ops = _encode(native, device_tables, 1, frames, [(0, 0, 1, 5), (0, 1, 1, 3)], [(1, 1)], O, wave=wave)
    assert (ops[0][:, 0] == 32).all() and (ops[0][:, 1:] == 0).all()
    assert enc.get_state(native.STATE_OUT_OF_WORK).tolist() == [1, 1]
    assert enc.get_state(native.STATE_COUNTERS)[:2].tolist() == [0, 0]


@pytest.mark.parametrize("mode,wave", [(1, True), (0, True), (1, False), (1, "shared"), (0, "shared")])
def test_constant_target_degenerate_priorities(native, O, oracle_tables, device_tables, mode, wave):
    """Every byte has the same priority (one histogram bucket): the prefix selection
    must fall back to ordering everything; ties are broken by nonce/page/offset only."""
    fr = np.zeros((1, 2, 2, 32, 256), np.uint8)
    fr[0, 0, :, :, :] = 0x55
    fr[0, 1, :, :, :] = 0x2a
    fr[..., HOLES] = 0
    sched = [(0, 0, 1, 200), (0, 1 if mode == 1 else 0, 1, 250), (1, 0, 1, 100), (1, 0, 1, 0)]
    enc, ops = _encode(native, device_tables, mode, fr, sched, [(3, 4)], O, wave=wave)
    v, exp = _oracle(O, oracle_tables, mode, fr[0], sched, (3, 4))
    assert (ops[0] == exp).all()
    assert (enc.get_state(native.STATE_UP_MAIN) == v.update_priority(0)).all()


@pytest.mark.parametrize("wave", [True, False, "shared"])
def test_few_changes_and_tiny_lists(native, O, oracle_tables, device_tables, wave):
    """Targets that differ from the screen in 0..70 bytes: lists shorter than one scan
    window, shorter than the opcode budget, exhaustion mid-segment, then padding."""
    rng = np.random.default_rng(11)
    n = 6
    fr = np.zeros((n, 2, 2, 32, 256), np.uint8)
    for i in range(n):
        k = [0, 1, 2, 7, 33, 70][i]
        for f in range(2):
            idx = rng.integers(0, 8192, k)
            for b in range(2):
                flat = fr[i, f, b].reshape(-1)
                flat[idx] = rng.integers(1, 128, k)
        fr[i][..., HOLES] = 0
    sched = [(0, 0, 1, 40), (0, 1, 1, 40), (1, 0, 1, 90), (1, 1, 1, 10), (1, 0, 1, 0)]
    seeds = [(i + 5, i + 50) for i in range(n)]
    enc, ops = _encode(native, device_tables, 1, fr, sched, seeds, O, wave=wave)
    for i in range(n):
        v, exp = _oracle(O, oracle_tables, 1, fr[i], sched, seeds[i])
        assert (ops[i] == exp).all(), i
        assert (enc.get_state(native.STATE_MEM_AUX, i) == v.memory(1)).all()
        cnt = enc.get_state(native.STATE_COUNTERS, i)
        assert (int(cnt[0]), int(cnt[1])) == v.draws()


def test_priorities_beyond_16_bits(native, O, oracle_tables, device_tables):
    """update_priority accumulates across calls and outgrows 16 bits: the
    64-bit keys must still order it, and the prefix selection must bucket it."""
    rng = np.random.default_rng(2)
    big = rng.integers(0, 300000, (32, 256)).astype(np.int32)
    # (the kernels keep a 16-bit copy whose largest value means "see the 32-bit array": values at and around that boundary,
    # and ones a single diff weight carries across it)
    big[3, :12] = [65533, 65534, 65535, 65536, 65537, 65535 - 2047, 65535 - 300, 65535 - 1, 131071, 131072, 1, 0]
    big[17, 100:110] = np.arange(65530, 65540)
    big[:, HOLES] = 0
    fr = rng.integers(0, 128, (1, 1, 2, 32, 256), dtype=np.uint8)
    fr[..., HOLES] = 0
    sched = [(0, 0, 1, 300), (0, 1, 1, 120), (0, 0, 1, 0)]

    def init_dev(enc):
        enc.set_state(native.STATE_UP_MAIN, big)

    def init_orc(v):
        v.update_priority(0)[...] = big

    for wave in (True, False):
        enc, ops = _encode(native, device_tables, 1, fr, sched, [(8, 9)], O, wave=wave, init=init_dev)
        v, exp = _oracle(O, oracle_tables, 1, fr[0], sched, (8, 9), init=init_orc)
        assert (ops[0] == exp).all()
        assert (enc.get_state(native.STATE_UP_MAIN) == v.update_priority(0)).all()


def test_prefix_sort_boundary_budgets(native, O, oracle_tables, device_tables):
    """Opcode budgets right at the prefix-sort limit (3 x 682 = 2046 <= 2048 < 3 x 683)
    and a continued generator whose total is only known from the segment list."""
    rng = np.random.default_rng(4)
    fr = rng.integers(0, 256, (2, 3, 2, 32, 256), dtype=np.uint8)
    fr[..., HOLES] = 0
    sched = [(0, 0, 1, 682), (1, 0, 1, 683), (2, 0, 1, 300), (2, 0, 0, 382), (2, 0, 1, 1)]
    seeds = [(1, 2), (3, 4)]
    enc, ops = _encode(native, device_tables, 0, fr, sched, seeds, O, wave=True)
    for i in range(2):
        v, exp = _oracle(O, oracle_tables, 0, fr[i], sched, seeds[i])
        assert (ops[i] == exp).all()


def test_full_size_batch_properties(native, O, oracle_tables, device_tables):
    """4096 streams x 3 frames (the bench's batch shape).  Size-independent checks:
    replaying each opcode stream onto a blank screen reproduces the device's memory
    maps; every store lands on a non-hole byte with the target's content; the batch is
    deterministic; and sampled streams equal their stand-alone oracle runs."""
    import torch
    import stream_batch
    S, F = 4096, 3
    t, s = device_tables.get(1)
    fm, fa = stream_batch.synth_frames_torch(S, F, True, seed=123)
    seeds = [(i + 1, i + 7) for i in range(S)]
    runs = []
    for rep in range(2):
        b = stream_batch.StreamBatch(1, t, s, S, seeds=seeds, dm=device_tables.dm[(1, 5)])
        ops, segs = b.encode_frames(fm, fa, F)
        b.enc.check()
        runs.append(ops.cpu().numpy())
        if rep == 0:
            mem_main = np.stack([b.enc.get_state(native.STATE_MEM_MAIN, i) for i in range(0, S, 97)])
            mem_aux = np.stack([b.enc.get_state(native.STATE_MEM_AUX, i) for i in range(0, S, 97)])
        b.close()
    assert np.array_equal(runs[0], runs[1])          # deterministic
    ops = runs[0]
    assert ops.shape == (S, sum(g[3] for g in segs), 6)
    assert (ops[:, :, 0] >= 32).all() and (ops[:, :, 0] < 64).all()
    assert not HOLES[ops[:, :, 2:6]].any()            # no store into a screen hole
    tm, ta = fm.cpu().numpy(), fa.cpu().numpy()
    for k, i in enumerate(range(0, S, 97)):
        cur = [np.zeros((32, 256), np.uint8), np.zeros((32, 256), np.uint8)]
        pos = 0
        for (f, ia, _, n) in segs:
            tgt = ta[i, f] if ia else tm[i, f]
            o = ops[i, pos:pos + n]
            assert (o[:, 1] == tgt[o[:, 0] - 32, o[:, 2]]).all()   # content = target byte of the primary
            bank = cur[ia]
            for row in o:                                          # in order: a byte can be stored
                bank[row[0] - 32, row[2:6]] = row[1]               # again later with another content
            pos += n
        assert np.array_equal(cur[0], mem_main[k]) and np.array_equal(cur[1], mem_aux[k])
    for i in (0, 1500, 4095):
        v, exp = _oracle(O, oracle_tables, 1, np.stack([tm[i], ta[i]], axis=1), segs, seeds[i])
        assert np.array_equal(ops[i], exp), i


@pytest.mark.parametrize("mode", [1, 0])
def test_kernel_forms_agree_at_batch_sizes(native, O, oracle_tables, device_tables, mode):
    """The kernel forms against each other at the sizes they are dispatched for, on picture-like input (ties on nearly
    every step): 600 clips through the eight-wave kernel and 4608 clips through the LDS-shared form (persistent
    workgroups taking streams off a queue, a partly filled last workgroup) both equal the plain one-wave kernel, opcode for
    opcode and in the final state; three sampled clips equal the oracle."""
    import stream_batch
    F = 3
    t, s = device_tables.get(mode)
    for S, other in ((600, "team"), (4608 + 5, "shared")):
        fm, fa = stream_batch.synth_frames_img(S, F, mode == 1, seed=900 + S)
        seeds = [(i + 1, i + 7) for i in range(S)]
        res = {}
        for kern in ("plain", other):
            b = stream_batch.StreamBatch(mode, t, s, S, seeds=seeds, dm=device_tables.dm[(mode, 5)])
            b.enc.set_greedy_kernel(kern)
            ops, segs = b.encode_frames(fm, fa, F)
            b.enc.check()
            up = np.stack([b.enc.get_state(native.STATE_UP_MAIN, i) for i in range(0, S, 151)])
            res[kern] = (ops.cpu().numpy(), up)
            b.close()
        assert np.array_equal(res["plain"][0], res[other][0]), (S, other)
        assert np.array_equal(res["plain"][1], res[other][1]), (S, other)
        tm = fm.cpu().numpy()
        ta = fa.cpu().numpy() if fa is not None else None
        for i in (0, S // 2, S - 1):
            fr = np.stack([tm[i], ta[i] if ta is not None else np.zeros_like(tm[i])], axis=1)
            v, exp = _oracle(O, oracle_tables, mode, fr, segs, seeds[i])
            assert np.array_equal(res[other][0][i], exp), (S, other, i)


@pytest.mark.parametrize("mode", [1, 0])
def test_encoder_picks_the_kernel_form_by_what_its_kernels_report(native, device_tables, mode):
    """A batch that fills the GPU runs the LDS-shared form of the one-wave kernel unless the kernels report input whose
    steps are mostly decided by the nonces -- more than 85 % of them (DHGR) / 30 % (HGR): include/iivision.h,
    iiv_encoder_input_stats -- where the plain form is the faster one.  The report
    travels by an asynchronous copy, so the choice follows a call or two behind; the bytes are the same either way
    (test_kernel_forms_agree_at_batch_sizes), only the rate differs."""
    import torch
    import stream_batch
    S, F = 4608, 4
    t, s = device_tables.get(mode)
    for kind, want_form, lo, hi in (("iid", "shared", 0.0, 0.15), ("img", "plain", 0.6, 1.0)):
        fm, fa = (stream_batch.synth_frames_img(S, F, mode == 1, seed=5) if kind == "img" else
                  stream_batch.synth_frames_torch(S, F, mode == 1, seed=5))
        b = stream_batch.StreamBatch(mode, t, s, S, seeds=[(i + 1, i + 1) for i in range(S)], dm=device_tables.dm[(mode, 5)])
        assert b.enc.input_stats()[0] == 0.0                    # nothing reported yet
        for f in range(F):
            b.encode_frames(fm, fa, 1)
            torch.cuda.synchronize()                            # (lets the copy behind each call land before the next looks)
        b.enc.check()
        share, form = b.enc.input_stats()
        assert lo <= share <= hi, (kind, share)
        if kind == "img":     # (these few frames from an empty screen tie at 60-100 % of the steps: the rule, not a fixed answer)
            want_form = "plain" if share > (0.85 if mode == 1 else 0.30) else "shared"
        assert form == want_form, (kind, share, form)
        # an explicit choice overrules the report
        b.enc.set_greedy_kernel("plain")
        assert b.enc.input_stats()[1] == "plain"
        b.enc.set_greedy_kernel("shared")
        assert b.enc.input_stats()[1] == "shared"
        b.close()


def test_bench_batch_size_sampled_against_the_oracle(native, O, oracle_tables, device_tables):
    """The bench's own batch -- 14336 DHGR streams, the persistent workgroups' queue running 3.5 rounds -- for two
    Movie-paced frames (three generators, a bank flip) through the one-wave kernel's forms: plain, LDS-shared, and both
    with the fourth offset.  Sixteen streams spread over the whole queue (first, last, the workgroup boundaries around the
    resident count) equal their stand-alone oracle runs opcode for opcode; the two forms agree on EVERY stream."""
    import stream_batch
    S, F = 14336, 2
    t, s = device_tables.get(1)
    fm, fa = stream_batch.synth_frames_torch(S, F, True, seed=2025)
    seeds = [(i + 1, 3 * i + 7) for i in range(S)]
    sample = sorted({0, 1, 7, 8, 63, 4095, 4096, 4097, 7167, 7168, 8191, 8192, 12287, 12288, S // 2 + 1, S - 2, S - 1})
    tm, ta = fm[sample].cpu().numpy(), fa[sample].cpu().numpy()
    for fourth in (False, True):
        res = {}
        for kern in ("plain", "shared"):
            b = stream_batch.StreamBatch(1, t, s, S, seeds=seeds, dm=device_tables.dm[(1, 5)], fourth_offset=fourth)
            b.enc.set_greedy_kernel(kern)
            ops, segs = b.encode_frames(fm, fa, F)
            b.enc.check()
            res[kern] = ops.cpu().numpy()
            b.close()
        assert np.array_equal(res["plain"], res["shared"]), fourth
        for j, i in enumerate(sample):
            _, exp = H.oracle_run(O, oracle_tables, 1, 5, np.stack([tm[j], ta[j]], axis=1), segs, seeds[i], fourth=fourth)
            assert np.array_equal(res["shared"][i], exp), (fourth, i)


@pytest.mark.parametrize("kern", ["plain", "shared"])
def test_longest_first_launch_order_changes_no_byte(native, device_tables, kern):
    """IIV_OPT_STREAM_ORDER: from 2048 streams on the one-wave kernel launches its streams in the order of what their
    latest launches cost (re-sorted every fourth launch).  Streams are independent: five Movie-paced frames (13
    generators, three re-sorts) of 2304 picture-like clips -- whose costs differ by 2x -- give the same opcodes, screens
    and RNG positions with the ordering on and off."""
    import stream_batch
    S, F = 2304, 5
    t, s = device_tables.get(1)
    fm, fa = stream_batch.synth_frames_img(S, F, True, seed=77)
    seeds = [(i + 3, i + 5) for i in range(S)]
    res = {}
    for order in (True, False):
        b = stream_batch.StreamBatch(1, t, s, S, seeds=seeds, dm=device_tables.dm[(1, 5)])
        b.enc.set_greedy_kernel(kern)
        b.enc.set_stream_order(order)
        ops, segs = b.encode_frames(fm, fa, F)
        b.enc.check()
        res[order] = (ops.cpu().numpy(), [b.enc.get_state(native.STATE_MEM_MAIN, i) for i in (0, 1, S // 2, S - 1)],
                      [b.enc.get_state(native.STATE_RNG_PY, i) for i in (0, S - 1)])
        b.close()
    assert len(segs) >= 10
    assert np.array_equal(res[True][0], res[False][0])
    for a, c in zip(res[True][1] + res[True][2], res[False][1] + res[False][2]):
        assert np.array_equal(a, c)
