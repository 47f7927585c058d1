"""GPU: every entry point of include/iivision.h that takes a `stream`, called on a busy non-blocking side stream under the
probe of tests/stream_probe.py, against the models and the oracle -- never against the device's own default-stream output.
A launch, memset or copy issued on another stream than the caller's, scratch freed on the wrong stream, a host array read
after the call returned: each changes bytes here, and none of them changes a byte on the default stream the rest of the
suite runs on."""
import ctypes as C

import numpy as np
import pytest

import a2m_model
import audio_model
import diffusion_model
import ingest_model
import mono_model
import render_error_model
import render_model
import resize_model
from stream_cases import Enc as _Enc, dp as _dp, frames as _frames, g6_addresses, maps as _maps, next_draws as _next_draws
from a2m_model import random_ops
from device_guards import ok
from encode_harness import seed_states as _seed_states
from stream_probe import Probe

pytestmark = pytest.mark.gpu

HGR, DHGR = 0, 1
MODES = [DHGR, HGR]


def _np(t):
    return t.cpu().numpy()


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- ingest and frames ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def colour_frames(O):
    real = ingest_model.frame_set(O.PALETTE_RGB[5], 41)[:5]
    return real, np.ascontiguousarray(np.roll(real, 1, axis=0))      # the decoy: the same frames, every one in another place


@pytest.mark.parametrize("dither", [32, 256])
@pytest.mark.parametrize("mode", MODES)
def test_colour_ingest(native, O, colour_frames, mode, dither):
    L = native.lib()
    real, decoy = colour_frames
    exp = [O.frame_to_memory_map(mode, O.PALETTE_RGB[5], f, dither) for f in real]
    p = Probe()
    rgb = p.input(real, decoy)
    main, aux = p.output((5, 32, 256)), p.output((5, 32, 256))
    pal = p.host(np.asarray(O.PALETTE_RGB[5], np.uint8).reshape(48), np.asarray(O.PALETTE_RGB[0], np.uint8).reshape(48))

    def call(st):
        ok(native, L.iiv_frames_to_memory_maps(mode, _hp(pal), 5, _dp(rgb), dither, _dp(main), _dp(aux), st))
    call(native.stream_ptr())
    p.run(call)
    assert np.array_equal(_np(main), np.stack([e[0] for e in exp]))
    assert np.array_equal(_np(aux), np.stack([e[1] for e in exp]) if mode == DHGR else Probe.sentinel((5, 32, 256)))


@pytest.fixture(scope="module")
def atkinson(O, colour_frames):
    w, div = diffusion_model.KERNELS["atkinson"]
    return {mode: diffusion_model.frames_to_memory_maps(mode, O.PALETTE_RGB[5], colour_frames[0], w, div) for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
def test_diffused_ingest(native, O, colour_frames, atkinson, mode):
    L = native.lib()
    real, decoy = colour_frames
    w, div = diffusion_model.KERNELS["atkinson"]
    lite, _ = diffusion_model.KERNELS["sierra-lite"]                  # sums to 4: legal under Atkinson's divisor 8 as well
    p = Probe()
    rgb = p.input(real, decoy)
    main, aux = p.output((5, 32, 256)), p.output((5, 32, 256))
    pal = p.host(np.asarray(O.PALETTE_RGB[5], np.uint8).reshape(48), np.asarray(O.PALETTE_RGB[0], np.uint8).reshape(48))
    wt = p.host(w.astype(np.uint8).reshape(15), lite.astype(np.uint8).reshape(15))

    def call(st):
        ok(native, L.iiv_frames_to_memory_maps_diffused(mode, _hp(pal), 5, _dp(rgb), _hp(wt), div, _dp(main), _dp(aux), st))
    call(native.stream_ptr())
    p.run(call)
    em, ea = atkinson[mode]
    assert np.array_equal(_np(main), em)
    assert np.array_equal(_np(aux), ea if mode == DHGR else Probe.sentinel((5, 32, 256)))


@pytest.mark.parametrize("dither", [32, 256])
@pytest.mark.parametrize("mode", MODES)
def test_mono_ingest(native, mode, dither):
    L = native.lib()
    real = mono_model.noise_frames(mode, 5, seed=7)
    real[3:] = mono_model.structured_frames(mode, 2, seed=3)
    em, ea = mono_model.frames_to_memory_maps(mode, real, dither)
    p = Probe()
    rgb = p.input(real, np.roll(real, 2, axis=0))
    main, aux = p.output((5, 32, 256)), p.output((5, 32, 256))

    def call(st):
        ok(native, L.iiv_frames_to_memory_maps_mono(mode, 5, _dp(rgb), dither, _dp(main), _dp(aux), st))
    call(native.stream_ptr())
    p.run(call)
    assert np.array_equal(_np(main), em)
    assert np.array_equal(_np(aux), ea if mode == DHGR else Probe.sentinel((5, 32, 256)))


def test_resize(native):
    L = native.lib()
    rng = np.random.default_rng(5)
    real = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    p = Probe()
    src = p.input(real, rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8))
    dst = p.output((3, 192, 280, 3))

    def call(st):
        ok(native, L.iiv_resize_frames(3, 37, 53, _dp(src), 37 * 53 * 3, 53 * 3, 192, 280, _dp(dst), st))
    call(native.stream_ptr())                                         # the first use of a size pair uploads its tables
    p.run(call)
    assert np.array_equal(_np(dst), resize_model.resize(real, (192, 280)))


# ---- rendering -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_render_rgb(native, O, mode):
    L = native.lib()
    rng = np.random.default_rng(11 + mode)
    rm, ra = _maps(rng, 3, mode), _maps(rng, 3, mode)
    p = Probe()
    main, aux = p.input(rm, _maps(rng, 3, mode)), p.input(ra, _maps(rng, 3, mode))
    out = p.output((3, 192, 560, 3))
    pal = p.host(np.asarray(O.PALETTE_RGB[5], np.uint8).reshape(48), np.asarray(O.PALETTE_RGB[0], np.uint8).reshape(48))

    def call(st):
        ok(native, L.iiv_render_rgb(mode, _hp(pal), 3, _dp(main), _dp(aux), _dp(out), st))
    call(native.stream_ptr())
    p.run(call)
    assert np.array_equal(_np(out), render_model.render_rgb(mode, rm, ra if mode == DHGR else None, O.PALETTE_RGB[5]))


@pytest.mark.parametrize("width", [560, 280])
@pytest.mark.parametrize("mode", MODES)
def test_render_error(native, O, mode, width):
    import torch
    L = native.lib()
    rng = np.random.default_rng(17 + mode + width)
    rm, ra = _maps(rng, 3, mode), _maps(rng, 3, mode)
    rref = rng.integers(0, 256, (3, 192, width, 3), dtype=np.uint8)
    p = Probe()
    main, aux = p.input(rm, _maps(rng, 3, mode)), p.input(ra, _maps(rng, 3, mode))
    ref = p.input(rref, rng.integers(0, 256, (3, 192, width, 3), dtype=np.uint8))
    out = p.output((3, 3, 3), torch.uint64)
    pal = p.host(np.asarray(O.PALETTE_RGB[5], np.uint8).reshape(48), np.asarray(O.PALETTE_RGB[0], np.uint8).reshape(48))

    def call(st):
        ok(native, L.iiv_render_error(mode, _hp(pal), 3, _dp(main), _dp(aux), _dp(ref), width, _dp(out), st))
    call(native.stream_ptr())
    p.run(call)
    exp = render_error_model.render_error(mode, rm, ra if mode == DHGR else None, O.PALETTE_RGB[5], rref)
    assert np.array_equal(_np(Probe.bytes_of(out)).view(np.uint64).reshape(3, 3, 3), exp)


# ---- the encoder ---------------------------------------------------------------------------------------------------

def _schedule(mode):
    b = 1 if mode == DHGR else 0
    return [(0, 0, 1, 120), (1, b, 1, 90), (1, b, 0, 40)]


SCRIBBLE_SEGMENTS = [(1, 0, 1, 100), (0, 0, 1, 60), (0, 0, 0, 20)]     # other frames, in range, no larger opcode counts


def _segment_arrays(native, segments, scribble):
    """(ctypes array handed to the library, a function that scribbles over it)"""
    arr = native.segment_array(segments)

    def scribble_now():
        for j, (f, a, r, k) in enumerate(scribble):
            arr[j].frame, arr[j].is_aux, arr[j].restart, arr[j].n_ops = f, a, r, k
    return arr, scribble_now


# every greedy launch line: name -> (encoder options, the kernel iiv_encoder_launch_forms must report, and no other)
FORMS = {"plain": (dict(kernel="plain"), "plain"), "shared": (dict(kernel="shared"), "shared"), "team": (dict(kernel="team"), "team"),
         "workgroup-joint": (dict(joint=True), "workgroup"), "fourth-team": (dict(kernel="team", fourth=True), "team"),
         "fourth-plain": (dict(kernel="plain", fourth=True), "plain"), "fourth-shared": (dict(kernel="shared", fourth=True), "shared"),
         # (csrc/iiv_launch_choice.h: the fourth offset overrides the kernel option; the LDS-shared form takes all of a CU's LDS)
         "workgroup": (dict(kernel="workgroup"), "workgroup"), "fourth-workgroup": (dict(kernel="workgroup", fourth=True), "plain"),
         "shared-lds-pad": (dict(kernel="shared", lds_pad=1024), "plain")}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("mode", MODES)
def test_encode(native, O, device_tables, oracle_tables, mode, form):
    L = native.lib()
    n, segments = 4, _schedule(mode)
    total = sum(s[3] for s in segments)
    fm, fa = _frames(mode, n, 2, 300 + mode)
    dm_, da_ = _frames(mode, n, 2, 400 + mode)
    options, kernel = FORMS[form]
    e = _Enc(native, O, device_tables, oracle_tables, mode, n, 21, **options)
    p = Probe()
    d_main, d_aux = p.input(fm, dm_), p.input(fa, da_)
    ops = p.output((n, total, 6))
    segs, scribble = _segment_arrays(native, segments, SCRIBBLE_SEGMENTS)
    p.scribble(scribble)

    def call(st):
        ok(native, L.iiv_encode(e.enc._h, _dp(d_main), _dp(d_aux if mode == DHGR else None), 2, segs, len(segments), _dp(ops), st))
    e.warm(call)
    e.enc.profile(True)
    p.run(call)
    e.enc.check()
    ran = e.enc.launch_forms()
    assert ran[kernel] > 0 and sum(ran.values()) == ran[kernel], (form, ran)
    got = _np(ops)
    for i in range(n):
        assert np.array_equal(got[i], e.oracle(i, fm, fa, segments)), (form, i)
    e.check_state()
    e.close()


def _encode_streams(native, O, device_tables, oracle_tables, mode, scheds, seed0, options={}, kernel=None):
    """iiv_encode_streams of four streams' schedules on the side stream; kernel: the one every greedy launch must have run"""
    L = native.lib()
    n = 4
    flat = [g for s in scheds for g in s]
    begin_real = np.concatenate([[0], np.cumsum([len(s) for s in scheds])]).astype(np.int32)
    width = max(sum(g[3] for g in s) for s in scheds)
    fm, fa = _frames(mode, n, 2, 500 + mode)
    dm_, da_ = _frames(mode, n, 2, 600 + mode)
    e = _Enc(native, O, device_tables, oracle_tables, mode, n, seed0, **options)
    p = Probe()
    d_main, d_aux = p.input(fm, dm_), p.input(fa, da_)
    ops = p.output((n, width, 6))
    begin = p.host(begin_real, np.zeros(n + 1, np.int32))             # every stream empty: a valid, other batch
    segs, scribble = _segment_arrays(native, flat, [(1 - f, 0, 1, max(k // 2, 1)) for (f, a, r, k) in flat])
    p.scribble(scribble)

    def call(st):
        ok(native, L.iiv_encode_streams(e.enc._h, _dp(d_main), _dp(d_aux if mode == DHGR else None), 2, segs,
                                        begin.ctypes.data_as(C.POINTER(C.c_int32)), _dp(ops), width * 6, st))
    e.warm(call)
    e.enc.profile(kernel is not None)
    p.run(call)
    e.enc.check()
    ran = e.enc.launch_forms()
    assert kernel is None or (ran[kernel] > 0 and sum(ran.values()) == ran[kernel]), ran
    got = _np(ops)
    for i in range(n):
        exp = e.oracle(i, fm, fa, scheds[i])
        assert np.array_equal(got[i, :len(exp)], exp), i
        assert (got[i, len(exp):] == 0x5B).all(), "stream %d wrote behind its own opcodes" % i
    e.check_state()
    e.close()


@pytest.mark.parametrize("mode", MODES)
def test_encode_streams(native, O, device_tables, oracle_tables, mode):
    b = 1 if mode == DHGR else 0
    _encode_streams(native, O, device_tables, oracle_tables, mode,
                    [[(0, 0, 1, 120), (1, b, 1, 90)], [], [(1, 0, 1, 70), (1, 0, 0, 30), (0, b, 1, 200)], [(0, b, 1, 33)]], 31)


def test_encode_streams_whose_rounds_mix_banks_run_the_plain_form(native, O, device_tables, oracle_tables):
    """DHGR under kernel="shared": in both rounds some streams work on the main bank and some on aux, and the LDS-shared form
    holds one bank's table per workgroup -- every launch is the plain form's (csrc/iiv_launch_choice.h), the bytes the oracle's"""
    _encode_streams(native, O, device_tables, oracle_tables, DHGR,
                    [[(0, 0, 1, 120), (1, 1, 1, 90)], [(0, 1, 1, 100), (1, 0, 1, 60)], [(1, 0, 1, 70)], [(0, 1, 1, 33)]], 35,
                    dict(kernel="shared"), "plain")


@pytest.mark.parametrize("mode", MODES)
def test_snapshot_and_rollback_between_encodes(native, O, device_tables, oracle_tables, mode):
    """encode A, snapshot, encode B, rollback, encode B again, no host synchronisation of the test's between them; both B's are the
    oracle's B.  (`busy` is taken once, behind the last call: the library's third encode of a chain waits on the host for the
    descriptor copy of the first -- its staging ring has two slots -- and this probe cannot see that wait.)"""
    L = native.lib()
    n = 2
    b = 1 if mode == DHGR else 0
    seg_a, seg_b = [(0, 0, 1, 150)], [(1, b, 1, 130), (1, b, 0, 25)]
    fm, fa = _frames(mode, n, 2, 700 + mode)
    dm_, da_ = _frames(mode, n, 2, 800 + mode)
    e = _Enc(native, O, device_tables, oracle_tables, mode, n, 41)
    p = Probe()
    d_main, d_aux = p.input(fm, dm_), p.input(fa, da_)
    oa, ob1, ob2 = p.output((n, 150, 6)), p.output((n, 155, 6)), p.output((n, 155, 6))
    sa, sb = native.segment_array(seg_a), native.segment_array(seg_b)
    aux = (lambda: _dp(d_aux)) if mode == DHGR else (lambda: C.c_void_p(0))

    def call(st):
        ok(native, L.iiv_encode(e.enc._h, _dp(d_main), aux(), 2, sa, 1, _dp(oa), st))
        ok(native, L.iiv_encoder_snapshot(e.enc._h, st))
        ok(native, L.iiv_encode(e.enc._h, _dp(d_main), aux(), 2, sb, 2, _dp(ob1), st))
        ok(native, L.iiv_encoder_rollback(e.enc._h, st))
        ok(native, L.iiv_encode(e.enc._h, _dp(d_main), aux(), 2, sb, 2, _dp(ob2), st))
    e.warm(call)
    p.run(call)
    e.enc.check()
    for i in range(n):
        assert np.array_equal(_np(oa)[i], e.oracle(i, fm, fa, seg_a)), i
        exp_b = e.oracle(i, fm, fa, seg_b)
        assert np.array_equal(_np(ob1)[i], exp_b) and np.array_equal(_np(ob2)[i], exp_b), i
    e.check_state()
    e.close()


def test_async_state_calls_around_an_encode(native, O, device_tables, oracle_tables):
    """set_state_async (both RNG states, out-of-work) -> encode -> get_video_brief_async into pinned memory, all enqueued"""
    import torch
    L = native.lib()
    mode, n = DHGR, 2
    segments = [(0, 0, 1, 200), (1, 1, 1, 60)]
    fm, fa = _frames(mode, n, 2, 900)
    dm_, da_ = _frames(mode, n, 2, 901)
    e = _Enc(native, O, device_tables, oracle_tables, mode, n, 51)
    p = Probe()
    d_main, d_aux = p.input(fm, dm_), p.input(fa, da_)
    ops = p.output((n, 260, 6))
    segs, scribble = _segment_arrays(native, segments, [(1, 0, 1, 100), (0, 0, 1, 60)])
    p.scribble(scribble)
    py, npw = _seed_states(O, 77, 78)
    py_other, np_other = _seed_states(O, 5, 6)
    h_py, h_np = p.host(py, py_other), p.host(npw, np_other)
    h_oow = p.host(np.array([0, 0], np.int32), np.array([1, 1], np.int32))
    pinned = torch.zeros(C.sizeof(native.VideoBrief), dtype=torch.uint8).pin_memory()
    brief = native.VideoBrief.from_address(pinned.data_ptr())

    def call(st):
        for what, a in ((native.STATE_RNG_PY, h_py), (native.STATE_RNG_NP, h_np), (native.STATE_OUT_OF_WORK, h_oow)):
            ok(native, L.iiv_encoder_set_state_async(e.enc._h, 1, what, _hp(a), a.nbytes, st))
        ok(native, L.iiv_encode(e.enc._h, _dp(d_main), _dp(d_aux), 2, segs, 2, _dp(ops), st))
        ok(native, L.iiv_encoder_get_video_brief_async(e.enc._h, 1, C.byref(brief), st))
    e.warm(call)
    C.memset(pinned.data_ptr(), 0, C.sizeof(native.VideoBrief))
    p.run(call)
    e.enc.check()
    L_o = O.lib()
    L_o.orc_mt_seed_py(L_o.orc_video_rng_py(e.videos[1]._h), 77)      # stream 1 runs under the seeds that were set in stream order
    L_o.orc_mt_seed_np(L_o.orc_video_rng_np(e.videos[1]._h), 78)
    for i in range(n):
        assert np.array_equal(_np(ops)[i], e.oracle(i, fm, fa, segments)), i
    e.check_state(counters=False)       # (stream 1 was re-seeded in stream order: the counters count from creation)
    full = e.enc.get_video_state(1)
    v = e.videos[1]
    assert np.array_equal(np.frombuffer(brief.rng_py, np.uint32), np.frombuffer(full.rng_py, np.uint32))
    assert np.array_equal(np.frombuffer(brief.rng_np, np.uint32), np.frombuffer(full.rng_np, np.uint32))
    assert list(brief.out_of_work) == list(full.out_of_work) == [int(v.out_of_work(0)), int(v.out_of_work(1))]
    assert list(brief.priority_sum) == [int(v.update_priority(0).sum()), int(v.update_priority(1).sum())]
    assert list(brief.hole_bytes) == [0, 0]
    assert _next_draws(O, np.frombuffer(brief.rng_py, np.uint32), 4, True) == _next_draws(O, v.rng_py().state_words(), 4, True)
    assert _next_draws(O, np.frombuffer(brief.rng_np, np.uint32), 4, False) == _next_draws(O, v.rng_np().state_words(), 4, False)
    e.close()


@pytest.mark.parametrize("mode", MODES)
def test_encoder_render_and_error_behind_an_encode(native, O, device_tables, oracle_tables, mode):
    """the screen AFTER the encode enqueued in front of them on the same stream, with no host synchronisation"""
    import torch
    L = native.lib()
    n = 2
    segments = _schedule(mode)
    total = sum(s[3] for s in segments)
    fm, fa = _frames(mode, n, 2, 1000 + mode)
    dm_, da_ = _frames(mode, n, 2, 1100 + mode)
    rng = np.random.default_rng(3)
    rref = rng.integers(0, 256, (n, 192, 280, 3), dtype=np.uint8)
    e = _Enc(native, O, device_tables, oracle_tables, mode, n, 61)
    p = Probe()
    d_main, d_aux = p.input(fm, dm_), p.input(fa, da_)
    ref = p.input(rref, rng.integers(0, 256, (n, 192, 280, 3), dtype=np.uint8))
    ops, rgb, err = p.output((n, total, 6)), p.output((n, 192, 560, 3)), p.output((n, 3, 3), torch.uint64)
    pal = p.host(np.asarray(O.PALETTE_RGB[5], np.uint8).reshape(48), np.asarray(O.PALETTE_RGB[0], np.uint8).reshape(48))
    segs = native.segment_array(segments)

    def call(st):
        ok(native, L.iiv_encode(e.enc._h, _dp(d_main), _dp(d_aux if mode == DHGR else None), 2, segs, len(segments), _dp(ops), st))
        ok(native, L.iiv_encoder_render(e.enc._h, 0, n, _hp(pal), _dp(rgb), st))
        ok(native, L.iiv_encoder_render_error(e.enc._h, 0, n, _hp(pal), _dp(ref), 280, _dp(err), st))
    e.warm(call)
    p.run(call)
    e.enc.check()
    for i in range(n):
        assert np.array_equal(_np(ops)[i], e.oracle(i, fm, fa, segments)), i
    mem = np.stack([v.memory(0) for v in e.videos])
    mem_aux = np.stack([v.memory(1) for v in e.videos]) if mode == DHGR else None
    assert np.array_equal(_np(rgb), render_model.render_rgb(mode, mem, mem_aux, O.PALETTE_RGB[5]))
    assert np.array_equal(_np(Probe.bytes_of(err)).view(np.uint64).reshape(n, 3, 3),
                          render_error_model.render_error(mode, mem, mem_aux, O.PALETTE_RGB[5], rref))
    e.close()


def test_encoder_check_waits_for_the_stream(native, O, device_tables, oracle_tables):
    """iiv_encoder_check synchronises: behind a sleeping stream it reports what the encode of the REAL frames ran into (a DHGR
    content byte with the palette bit set, video.py:137) -- the decoy frames are clean."""
    L = native.lib()
    fm, fa = _frames(DHGR, 1, 1, 1200)
    bad = fm.copy()
    bad[0, 0, np.arange(64) % 32, (np.arange(64) * 37) % 120] |= 0x80
    e = _Enc(native, O, device_tables, oracle_tables, DHGR, 1, 71)
    p = Probe()
    d_main, d_aux = p.input(bad, fm), p.input(fa, _frames(DHGR, 1, 1, 1201)[1])
    ops = p.output((1, 2048, 6))
    segs = native.segment_array([(0, 0, 1, 2048)])
    clean = native.segment_array([(0, 0, 1, 8)])
    ok(native, L.iiv_encode(e.enc._h, _dp(d_main), _dp(d_aux), 1, clean, 1, _dp(ops), native.stream_ptr()))   # warm-up, on the decoy
    e.enc.check()

    def call(st):
        ok(native, L.iiv_encode(e.enc._h, _dp(d_main), _dp(d_aux), 1, segs, 1, _dp(ops), st))
        return L.iiv_encoder_check(e.enc._h, None, st)
    assert p.run(call, asynchronous=False) == native.ERR_ASSERT
    e.close()


# ---- .a2m reading and writing ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def addresses(golden):
    return g6_addresses(golden)


def test_a2m_scan_decode_replay(native, O, addresses):
    """3 streams of 700 opcodes (ACKs after opcodes 290 and 582), scanned, decoded and replayed in one enqueued chain"""
    import torch
    L = native.lib()
    tick, ack, term = addresses
    rng = np.random.default_rng(21)
    S, n_ops, modes = 3, 700, (1, 0, 1)
    assert a2m_model.P(n_ops) > 2 * 2048

    def streams():
        return np.stack([O.emit_stream(modes[s], *random_ops(rng, n_ops), tick, ack, term) for s in range(S)])
    real, decoy = streams(), streams()
    stride = real.shape[1]
    max_ops = a2m_model.max_ops(stride)
    init = rng.integers(0, 256, (2, S, 32, 256), dtype=np.uint8)
    reader = native.A2mReaderHandle(tick, ack, term)
    p = Probe()
    data = p.input(real, decoy)
    im, ia = p.input(init[0], np.roll(init[0], 1, axis=0)), p.input(init[1], np.roll(init[1], 1, axis=0))
    lengths = torch.full((S,), stride, dtype=torch.int64, device="cuda")
    info = p.output((S, 4), torch.int64)
    ops, ticks, banks = p.output((S, max_ops, 6)), p.output((S, max_ops)), p.output((S, max_ops))
    main, aux = p.output((S, 3, 32, 256)), p.output((S, 3, 32, 256))

    def call(st):
        ok(native, L.iiv_a2m_scan(reader._h, S, _dp(data), stride, _dp(lengths), _dp(info), st))
        ok(native, L.iiv_a2m_decode(reader._h, S, _dp(data), stride, _dp(info), _dp(ops), max_ops * 6, _dp(ticks), _dp(banks),
                                    max_ops, st))
        ok(native, L.iiv_a2m_replay(reader._h, S, _dp(data), stride, _dp(info), 100, 300, 3, _dp(im), _dp(ia), _dp(main), _dp(aux), st))
    call(native.stream_ptr())
    p.run(call)
    g_info, g_ops, g_ticks, g_banks, g_main, g_aux = (_np(t) for t in (info, ops, ticks, banks, main, aux))
    for s in range(S):
        assert tuple(g_info[s]) == a2m_model.scan(real[s], tick, ack, term) == (a2m_model.OK, modes[s], n_ops, 0), s
        _, m_ops, m_ticks, m_banks = a2m_model.decode(real[s], tick, ack, term)
        assert np.array_equal(g_ops[s, :n_ops], m_ops) and (g_ops[s, n_ops:] == 0x5B).all(), s
        assert np.array_equal(g_ticks[s, :n_ops], m_ticks) and (g_ticks[s, n_ops:] == 0x5B).all(), s
        assert np.array_equal(g_banks[s, :n_ops], m_banks) and (g_banks[s, n_ops:] == 0x5B).all(), s
        m_main, m_aux = a2m_model.replay(real[s], tick, ack, term, first=100, every=300, n=3, init=(init[0, s], init[1, s]))
        assert np.array_equal(g_main[s], m_main) and np.array_equal(g_aux[s], m_aux), s
    reader.close()


@pytest.mark.parametrize("mode", MODES)
def test_emit_chunk(native, O, addresses, mode):
    """opcodes 250 .. 649 of 3 streams: the slice crosses the ACKs after opcodes 290 and 582"""
    L = native.lib()
    tick, ack, term = addresses
    rng = np.random.default_rng(31 + mode)
    S, first, n = 3, 250, 400
    full = [random_ops(rng, first + n) for _ in range(S)]
    other = [random_ops(rng, n) for _ in range(S)]
    p = Probe()
    ops = p.input(np.stack([o[first:] for o, _ in full]), np.stack([o for o, _ in other]))
    ticks = p.input(np.stack([t[first:] for _, t in full]), np.stack([t for _, t in other]))
    d_tick = p.input(tick.view(np.int16), np.ascontiguousarray(tick[::-1]).view(np.int16))
    b0, nb = C.c_size_t(0), C.c_size_t(0)
    ok(native, L.iiv_emit_chunk(mode, 1, first, n, None, 0, None, 0, 34, None, 0, None, 0, C.byref(b0), C.byref(nb), None, None))
    width = int(nb.value) + 16
    out = p.output((S, width))

    def call(st):
        ok(native, L.iiv_emit_chunk(mode, S, first, n, _dp(ops), n * 6, _dp(ticks), n, 34, _dp(d_tick), ack, _dp(out), width,
                                    C.byref(b0), C.byref(nb), None, st))
    call(native.stream_ptr())
    p.run(call)
    got = _np(out)
    for s in range(S):
        whole = O.emit_stream(mode, full[s][0], full[s][1], tick, ack, term)
        assert np.array_equal(got[s, :nb.value], whole[b0.value:b0.value + nb.value]), s
        assert (got[s, nb.value:] == 0x5B).all(), s
    assert a2m_model.P(first) == b0.value and b0.value < 2044 < 4092 < b0.value + nb.value


def test_emit_stream_waits_for_the_stream(native, O, addresses):
    """iiv_emit_stream synchronises: asleep in front of its inputs it still writes the real opcodes' bytes; tick_addr is a host
    array read before it returns"""
    L = native.lib()
    tick, ack, term = addresses
    rng = np.random.default_rng(41)
    S, n = 2, 650
    real, other = [random_ops(rng, n) for _ in range(S)], [random_ops(rng, n) for _ in range(S)]
    length = native.emit_stream_size(DHGR, n, tick, ack, term)
    p = Probe()
    ops = p.input(np.stack([o for o, _ in real]), np.stack([o for o, _ in other]))
    ticks = p.input(np.stack([t for _, t in real]), np.stack([t for _, t in other]))
    ta = p.host(tick, tick[::-1])
    out = p.output((S, length + 8))
    got_len = C.c_size_t(0)

    def call(st):
        ok(native, L.iiv_emit_stream(DHGR, S, n, _dp(ops), _dp(ticks), _hp(ta), ack, term, 0, _dp(out), length + 8, C.byref(got_len), st))
    p.run(call, asynchronous=False)
    assert got_len.value == length
    for s in range(S):
        assert np.array_equal(_np(out)[s, :length], O.emit_stream(DHGR, real[s][0], real[s][1], tick, ack, term)), s
        assert (_np(out)[s, length:] == 0x5B).all()


# ---- audio ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def audio():
    rng = np.random.default_rng(51)

    def pcm(n, ch, f0):
        t = np.arange(n) / 44100.0
        x = 9000 * np.sin(2 * np.pi * f0 * t)[:, None] * (1.0 - 0.3 * np.arange(ch)) + rng.normal(0, 1500, (n, ch))
        return np.clip(np.round(x), -32768, 32767).astype(np.int16)
    streams = [pcm(5000, 2, 440.0), pcm(3001, 1, 1234.0)]
    others = [pcm(5000, 2, 777.0), pcm(3001, 1, 99.0)]

    def rows(ps):
        host = np.zeros((2, 10000), np.int16)
        for s, q in enumerate(ps):
            host[s, :q.size] = q.reshape(-1)
        return host
    return streams, rows(streams), rows(others)


def _audio_host(p):
    """the host arrays of both audio calls, and what overwrites them: smaller frame counts, another layout and rate"""
    lng = np.dtype(C.c_long)
    return (p.host(np.array([5000, 3001], lng), np.array([1200, 900], lng)), p.host(np.array([2, 1], np.int32), np.array([1, 2], np.int32)),
            p.host(np.array([44100, 44100], np.int32), np.array([22050, 48000], np.int32)))


def test_audio_ticks(native, audio):
    from audio_model import check_ticks as _check_ticks
    L = native.lib()
    streams, real, decoy = audio
    norms = [audio_model.normalization(q.reshape(-1), q.shape[1], 44100) for q in streams]
    counts = [audio_model.tick_count(q.shape[0], 44100, block_frames=2048) for q in streams]
    stride = max(counts) + 64
    p = Probe()
    pcm = p.input(real, decoy)
    out = p.output((2, stride))
    nf, ch, rt = _audio_host(p)
    nm = p.host(np.array(norms, np.float64), np.array([1.0, 9.5]))
    got = np.zeros(2, np.dtype(C.c_long))

    def call(st):
        ok(native, L.iiv_audio_ticks(2, _dp(pcm), 10000, _hp(nf), _hp(ch), _hp(rt), 14700, 2048, _hp(nm), _dp(out), stride, _hp(got), st))
        return got.copy()
    call(native.stream_ptr())
    assert list(p.run(call)) == counts
    host = _np(out)
    for s, q in enumerate(streams):
        want, v = audio_model.ticks(q.reshape(-1), q.shape[1], 44100, norms[s], block_frames=2048)
        _check_ticks(host[s, :counts[s]], want, v)
        assert (host[s, counts[s]:] == 0x5B).all(), s


def test_audio_resample(native, audio):
    import torch
    L = native.lib()
    streams, real, decoy = audio
    lens = [audio_model.n_out(q.shape[0], 44100) for q in streams]
    stride = max(lens) + 16
    p = Probe()
    pcm = p.input(real, decoy)
    out = p.output((2, stride), torch.float32)
    nf, ch, rt = _audio_host(p)
    got = np.zeros(2, np.dtype(C.c_long))

    def call(st):
        ok(native, L.iiv_audio_resample(2, _dp(pcm), 10000, _hp(nf), _hp(ch), _hp(rt), 14700, _dp(out), stride, _hp(got), st))
        return got.copy()
    call(native.stream_ptr())
    assert list(p.run(call)) == lens
    host = _np(out)
    untouched = Probe.sentinel((1,), np.float32)[0]
    for s, q in enumerate(streams):
        want = audio_model.decode(q.reshape(-1), q.shape[1], 44100)
        assert np.abs(host[s, :lens[s]] - want).max() <= 1e-5 * np.abs(want).max(), s      # (test_gpu_audio's bound for one block)
        assert (host[s, lens[s]:].view(np.uint32) == untouched.view(np.uint32)).all(), s


def test_audio_normalization_waits_for_the_stream(native, audio):
    L = native.lib()
    streams, real, decoy = audio
    p = Probe()
    pcm = p.input(real, decoy)
    nf, ch, rt = _audio_host(p)
    got = np.zeros(2, np.float64)

    def call(st):
        ok(native, L.iiv_audio_normalization(2, _dp(pcm), 10000, _hp(nf), _hp(ch), _hp(rt), 14700, _hp(got), st))
        return got.copy()
    got_now = p.run(call, asynchronous=False)
    for s, q in enumerate(streams):
        want = audio_model.normalization(q.reshape(-1), q.shape[1], 44100)
        assert abs(got_now[s] - want) <= 1e-5 * abs(want), s                                # (test_gpu_audio's bound)


# ---- tables and bitmaps ----------------------------------------------------------------------------------------------

def test_cie2000_calls_on_a_sleeping_stream(native, O):
    """iiv_cie2000_matrix and iiv_delta_e_cie2000 synchronise; their inputs and outputs are host arrays (read and written by the
    time they return, whatever the stream is doing)"""
    L = native.lib()
    p = Probe()
    rgb = p.host(np.asarray(O.PALETTE_RGB[5], np.uint8).reshape(48), np.asarray(O.PALETTE_RGB[0], np.uint8).reshape(48))
    rng = np.random.default_rng(61)
    lab1 = np.column_stack([rng.uniform(0, 100, 40), rng.uniform(-100, 100, 40), rng.uniform(-100, 100, 40)])
    lab2 = np.column_stack([rng.uniform(0, 100, 40), rng.uniform(-100, 100, 40), rng.uniform(-100, 100, 40)])
    a, b = p.host(lab1, lab2), p.host(lab2, lab1 * 0.5)
    f, i, de = np.zeros((16, 16)), np.zeros((16, 16), np.int32), np.zeros(40)

    def call(st):
        ok(native, L.iiv_cie2000_matrix(_hp(rgb), _hp(f), _hp(i), st))
        ok(native, L.iiv_delta_e_cie2000(40, _hp(a), _hp(b), _hp(de), st))
        return f.copy(), i.copy(), de.copy()
    f, i, de = p.run(call, asynchronous=False)
    fo, io = O.cie2000_matrix(O.PALETTE_RGB[5])
    assert np.array_equal(i, io) and np.abs(f - fo).max() < 1e-5          # (the suite's bound for the float matrix: conftest)
    assert np.abs(de - O.delta_e_cie2000(lab1, lab2)).max() < 1e-5


@pytest.mark.parametrize("mode,name", [(DHGR, "DHGR"), (HGR, "HGR")])
def test_bitmap_operations(native, golden, device_tables, mode, name):
    """iiv_pack of two screens, iiv_diff_weights between them, iiv_compute_delta_pages: reference-recorded vectors"""
    import torch
    L = native.lib()
    g = golden.g4_bitmap_ops
    table, _ = device_tables.get(mode)
    mains = np.stack([g[name + "_src_main"], g[name + "_tgt_main"]])
    auxs = np.stack([g[name + "_src_aux"], g[name + "_tgt_aux"]])
    sp, tp = g[name + "_src_packed"].view(np.int64), g[name + "_tgt_packed"].view(np.int64)
    pages, contents = g[name + "_delta_pages_0"].astype(np.int32), g[name + "_delta_contents_0"].astype(np.int32)
    dw = g[name + "_dw_0"].astype(np.int32)
    k = len(pages)
    hi = 128 if mode == DHGR else 256
    p = Probe()
    d_main, d_aux = p.input(mains, mains[::-1]), p.input(auxs, auxs[::-1])
    d_src, d_tgt = p.input(sp[None], tp[None]), p.input(tp[None], sp[None])
    d_pages, d_contents = p.input(pages, (pages + 1) % 32), p.input(contents, (contents + 1) % hi)
    d_rows = p.input(dw[pages], dw[(pages + 1) % 32])
    packed, weights, delta = p.output((2, 32, 128), torch.int64), p.output((1, 32, 256), torch.int32), p.output((k, 256), torch.int32)

    def call(st):
        ok(native, L.iiv_pack(mode, 2, _dp(d_main), _dp(d_aux if mode == DHGR else None), _dp(packed), st))
        ok(native, L.iiv_diff_weights(mode, _dp(table), 1, _dp(d_src), _dp(d_tgt), 0, _dp(weights), st))
        ok(native, L.iiv_compute_delta_pages(mode, _dp(table), k, _dp(d_tgt), _dp(d_pages), _dp(d_contents), _dp(d_rows), 0,
                                             _dp(delta), st))
    call(native.stream_ptr())
    p.run(call)
    assert np.array_equal(_np(packed), np.stack([sp, tp]))
    assert np.array_equal(_np(weights)[0], dw)
    assert np.array_equal(_np(delta), g[name + "_delta_0"])


def test_tables_from_a_file_table(native, oracle_tables, device_tables):
    """iiv_symmetrise_table and iiv_store_table_from_table (HGR): the lower triangle a reference .npz holds, mirrored in place and
    turned into the store table on the side stream; the decoy is another lower triangle (every entry halved).  The mirrored table
    is held to the oracle's; there is no oracle store table, so the store table is held to iiv_build_store_table's, another
    kernel's output from the diff matrix, as tests/test_gpu_tables.py does."""
    import torch
    L = native.lib()
    otab = oracle_tables.get(HGR)
    full = torch.from_numpy(otab.view(np.int16)).cuda()
    idx = torch.arange(1 << 28, dtype=torch.int32, device="cuda")
    lower_mask = (idx >> 14) > (idx & 16383)
    del idx
    real = torch.where(lower_mask[None], full, torch.zeros((), dtype=torch.int16, device="cuda"))
    del lower_mask, full
    decoy = real >> 1
    p = Probe()
    table, keep = p.in_place(real, decoy)
    store = p.output((L.iiv_store_table_entries(HGR),), torch.int16)

    def call(st, t=None):
        t = table if t is None else t
        ok(native, L.iiv_symmetrise_table(HGR, _dp(t), st))
        ok(native, L.iiv_store_table_from_table(HGR, _dp(t), _dp(store), st))
    call(native.stream_ptr(), decoy.clone())                                                # warm-up, not on the probe's table
    p.run(call)
    assert np.array_equal(_np(keep).view(np.uint16), otab)
    _, dstore = device_tables.get(HGR)
    assert bool((store == dstore).all())
