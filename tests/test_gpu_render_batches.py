"""GPU: render_kernel (csrc/iiv_render.hip) and render_error_kernel (csrc/iiv_render_error.hip) past the first trip of their
grid-stride loops, as tests/test_gpu_resize_batches.py and tests/test_gpu_yuv_batches.py do for the host loops of the resize.

Both kernels walk a list of 64-unit runs, RUNS_PER_FRAME = 105 a frame, with a grid of at most GRID_CAP = 2048 workgroups of
RENDER_WAVES = 4 waves (render_grid in csrc/iiv_render.h): RUNS_PER_TRIP = 8192 runs a trip.  8192 / 105 = 78.02, so a wave
takes a second run only from 79 frames on, and a third from 157 (16384 / 105 = 156.04).  On a later trip a wave reuses its
private LDS behind three wave_lds_sync() calls and the zero margins it wrote once in front of the loop; in the error kernel
one wave then adds to the 72 output bytes of more than one frame, and frame 78 gets runs 8190, 8191 from the first trip and
its other 103 from the second.

Frame i of every batch is item i % 7 of a pool of seven -- a random screen pair and a random reference picture --, gathered
on the device with index_select; the models (tests/render_model.py, tests/render_error_model.py) run on the seven and EVERY
frame of the batch is compared.  A wave that starts at run r meets run r + 8192 k on trip k, which lies 78 or 79 frames (k = 1)
or 156 or 157 frames (k = 2) further on: 1, 2, 2 or 3 items further round the pool, never 0 -- asserted below --, so a trip
that computes with an earlier trip's frame, rows or sums computes another item's.  tests/test_render_batches_host.py holds the
seven items' expected outputs pairwise different, and the constants below equal to the header's, on the CPU.

Outputs are slices of larger buffers filled with a sentinel byte: an unwritten frame shows, and so does a byte written in front
of or behind the output."""
import ctypes as C
import functools

import numpy as np
import pytest

from device_guards import guarded, ok
import encode_harness as H
import render_error_model as E
import render_model as R
from stream_probe import Probe, SENTINEL_B
from test_gpu_render import DISTINCT, _palettes

pytestmark = pytest.mark.gpu

# mirrored from the library; tests/test_render_batches_host.py reads them from the sources' text and fails if they moved
RENDER_WAVES = 4            # csrc/iiv_render.h:21   constexpr int kRenderWaves = 4
RUNS_PER_FRAME = 105        # csrc/iiv_render.h:22   constexpr int kRenderRunsPerFrame = 105
GRID_CAP = 2048             # csrc/iiv_render.h:44   render_grid: blocks < 2048 ? blocks : 2048
RUNS_PER_TRIP = GRID_CAP * RENDER_WAVES     # csrc/iiv_render.hip:36, csrc/iiv_render_error.hip:54: n_waves = gridDim.x * kRenderWaves

P = 7                       # items in the pool
N_SECOND, N_THIRD = 79, 157  # the smallest batches with a second and with a third trip
MODES = [R.HGR, R.DHGR]
WIDTHS = [280, 560]
PALETTES = ["distinct", "NTSC", "IIGS", "MONO"]
FRAME = 192 * 560 * 3
GUARD = 0xA5
LEAD, TRAIL = 64 + 16, 64   # the output at 16 bytes and no more, as test_gpu_render.test_guards_and_least_alignments has it
OWN = (1, 3, 5)             # the pool items whose reference is their own rendering in the "own rendering" case; 78 % 7 = 1:
                            # the frame that straddles the first two trips is one of them
STREAM0_ITEM = 3            # what stream 0 of the 80-stream encoder shows: not item 0, which frame 0 of the range must be


def trips(n):
    """grid-stride trips the longest-running wave of an n-frame call makes"""
    return -(-n * RUNS_PER_FRAME // RUNS_PER_TRIP)


def assert_trips(n):
    """the arithmetic a case of n frames relies on"""
    assert n in (N_SECOND, N_THIRD)
    assert n * RUNS_PER_FRAME > GRID_CAP * RENDER_WAVES and (N_SECOND - 1) * RUNS_PER_FRAME <= GRID_CAP * RENDER_WAVES
    if n == N_THIRD:
        assert n * RUNS_PER_FRAME > 2 * GRID_CAP * RENDER_WAVES and (N_THIRD - 1) * RUNS_PER_FRAME <= 2 * GRID_CAP * RENDER_WAVES
    assert trips(n) == (3 if n == N_THIRD else 2)
    # the frame a wave meets on a later trip is never the pool item it had on an earlier one
    first = np.arange(RUNS_PER_TRIP)
    for k in range(1, trips(n)):
        for j in range(k):
            apart = (first + k * RUNS_PER_TRIP) // RUNS_PER_FRAME - (first + j * RUNS_PER_TRIP) // RUNS_PER_FRAME
            assert (apart % P != 0).all()
    assert (N_SECOND - 1) % P == 1
    # frame 78 has runs of the first trip and runs of the second
    assert (N_SECOND - 1) * RUNS_PER_FRAME < RUNS_PER_TRIP < N_SECOND * RUNS_PER_FRAME


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pool():
    """(main, aux, {280: ref, 560: ref}): seven random screen pairs (random bytes in the holes too), a random reference each"""
    rng = np.random.default_rng(7905)
    main = rng.integers(0, 256, (P, 32, 256), dtype=np.uint8)
    aux = rng.integers(0, 256, (P, 32, 256), dtype=np.uint8)
    refs = {w: _frozen(rng.integers(0, 256, (P, 192, w, 3), dtype=np.uint8)) for w in WIDTHS}
    return _frozen(main), _frozen(aux), refs


@functools.lru_cache(maxsize=None)
def want_rgb(mode, pal_name):
    """the model's rendering of the seven: computed once, shared, never written to"""
    main, aux, _ = pool()
    return _frozen(R.render_rgb(mode, main, aux, _palettes()[pal_name]))


@functools.lru_cache(maxsize=None)
def own_refs(mode, pal_name):
    """the 560-wide references with the items of OWN replaced by the model's own rendering of them"""
    ref = pool()[2][560].copy()
    ref[list(OWN)] = want_rgb(mode, pal_name)[list(OWN)]
    return _frozen(ref)


@functools.lru_cache(maxsize=None)
def want_sums(mode, width, pal_name, own=False):
    """the model's nine sums of the seven, (7, 3, 3) uint64"""
    ref = own_refs(mode, pal_name) if own else pool()[2][width]
    return _frozen(E.error_sums_of_screens(want_rgb(mode, pal_name), ref))


def _items(n, shift=0):
    return (np.arange(n) + shift) % P


def _gather(a, n):
    """CUDA frame i = a[i % P]: the pool uploaded, the batch built on the device"""
    import torch
    dev = torch.from_numpy(np.array(a)).cuda()
    return dev.index_select(0, torch.arange(n, device="cuda") % P)


def _check_every_frame(out, exp):
    """out: CUDA (n, ...); exp: numpy (P, ...) -- every frame i equals exp[i % P], compared on the device"""
    import torch
    n = out.shape[0]
    e = torch.from_numpy(np.array(exp)).to(out.device)
    bad = torch.zeros(n, dtype=torch.bool, device=out.device)
    for r in range(P):
        bad[r::P] = (out[r::P] != e[r]).flatten(1).any(1)
    idx = torch.nonzero(bad).flatten().cpu().numpy()
    assert len(idx) == 0, "%d of %d frames differ from the model, the first at %s" % (len(idx), n, idx[:10])


def _check_every_sum(got, exp, n):
    """got: numpy (n, 3, 3) uint64; exp: (P, 3, 3) -- all nine sums of every frame"""
    assert got.shape == (n, 3, 3) and got.dtype == np.uint64
    want = exp[_items(n)]
    bad = np.nonzero((got != want).reshape(n, 9).any(axis=1))[0]
    assert len(bad) == 0, "%d of %d frames' sums differ from the model, the first at %s: kernel %s, model %s" % (
        len(bad), n, bad[:10], got[bad[0]].tolist(), want[bad[0]].tolist())


def _all_hold(t, value):
    return bool((t == value).all())


def _sums_out(n, fill=0xFF):
    """a buffer of (n + 2) x 72 fill bytes and the (n, 3, 3) uint64 view of its middle"""
    import torch
    buf = torch.full(((n + 2) * 72,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[72:72 + n * 72].view(torch.uint64).view(n, 3, 3)


def _sums_guards_kept(buf, n, fill=0xFF):
    """the 72 bytes in front of frame 0's sums and the 72 behind frame n - 1's still hold the fill"""
    return _all_hold(buf[:72], fill) and _all_hold(buf[72 + n * 72:], fill)


# ---- iiv_render_rgb -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pal_name", PALETTES)
@pytest.mark.parametrize("n", [N_SECOND, N_THIRD])
@pytest.mark.parametrize("mode", MODES)
def test_render_rgb_every_frame_past_the_first_trip(native, mode, n, pal_name):
    assert_trips(n)
    main, aux, _ = pool()
    dm, da = _gather(main, n), _gather(aux, n)
    obuf, oview = guarded(n * FRAME, LEAD, TRAIL, GUARD)
    assert oview.data_ptr() % 32 == 16
    got = native.render_rgb(mode, _palettes()[pal_name], dm, da if mode == R.DHGR else None, out=oview)
    assert tuple(got.shape) == (n, 192, 560, 3)
    _check_every_frame(got, want_rgb(mode, pal_name))
    assert _all_hold(obuf[:LEAD], GUARD) and _all_hold(obuf[LEAD + n * FRAME:], GUARD)


# ---- iiv_render_error ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [N_SECOND, N_THIRD])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_render_error_every_sum_past_the_first_trip(native, mode, width, n):
    """All nine sums of every frame; the output starts as 0xFF bytes, so the call's own zeroing has to reach every frame, and
    the bytes in front of frame 0 and behind frame n - 1 keep them."""
    assert_trips(n)
    pal_name = "distinct" if n == N_SECOND else "NTSC"
    main, aux, refs = pool()
    dm, da, dr = _gather(main, n), _gather(aux, n), _gather(refs[width], n)
    buf, out = _sums_out(n)
    got = native.render_error(mode, _palettes()[pal_name], dm, da if mode == R.DHGR else None, dr, out=out)
    assert got.data_ptr() == out.data_ptr()
    _check_every_sum(got.cpu().numpy(), want_sums(mode, width, pal_name), n)
    assert _sums_guards_kept(buf, n)


@pytest.mark.parametrize("mode", MODES)
def test_own_rendering_reads_zero_wherever_its_runs_fell(native, mode):
    """The references of pool items 1, 3 and 5 are the model's rendering of those screens: their frames -- frame 78, whose runs
    fall into two trips, among them -- read exactly 0 in all nine sums, the others the model's sums, which are not 0."""
    n = N_SECOND
    assert_trips(n)
    assert (N_SECOND - 1) % P in OWN
    main, aux, _ = pool()
    want = want_sums(mode, 560, "distinct", own=True)
    zero = np.isin(np.arange(P), OWN)
    assert not want[zero].any() and want[~zero].all()
    dm, da, dr = _gather(main, n), _gather(aux, n), _gather(own_refs(mode, "distinct"), n)
    buf, out = _sums_out(n)
    got = native.render_error(mode, DISTINCT, dm, da if mode == R.DHGR else None, dr, out=out).cpu().numpy()
    assert not got[zero[_items(n)]].any(), np.nonzero(got.reshape(n, 9).any(axis=1) & zero[_items(n)])[0][:10]
    _check_every_sum(got, want, n)
    assert _sums_guards_kept(buf, n)


# ---- the encoder's own screens: frames one StreamState apart ---------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_encoder_render_and_render_error_over_79_of_80_streams(native, device_tables, mode):
    """iiv_encoder_render / iiv_encoder_render_error with first_stream = 1, n_streams = 79 on an encoder of 80 streams: stream
    1 + i shows pool item i % 7, stream 0 item 3 -- a range that started at stream 0 would put item 3 where item 0 belongs and
    every other frame one item late."""
    S, first, n = 80, 1, N_SECOND
    assert_trips(n)
    assert first + n == S and STREAM0_ITEM != 0
    main, aux, refs = pool()
    shown = np.concatenate([[STREAM0_ITEM], _items(n)])
    pal = _palettes()["NTSC"]
    enc = H.make_encoder(native, device_tables, mode, n_streams=S)
    try:
        enc.set_state_all(native.STATE_MEM_MAIN, main[shown])
        if mode == R.DHGR:
            enc.set_state_all(native.STATE_MEM_AUX, aux[shown])
        obuf, oview = guarded(n * FRAME, LEAD, TRAIL, GUARD)
        got = native.encoder_render(enc, pal, first_stream=first, n_streams=n, out=oview)
        _check_every_frame(got, want_rgb(mode, "NTSC"))
        assert _all_hold(obuf[:LEAD], GUARD) and _all_hold(obuf[LEAD + n * FRAME:], GUARD)
        for width in WIDTHS:
            buf, out = _sums_out(n)
            sums = native.encoder_render_error(enc, pal, _gather(refs[width], n), first_stream=first, n_streams=n, out=out)
            _check_every_sum(sums.cpu().numpy(), want_sums(mode, width, "NTSC"), n)
            assert _sums_guards_kept(buf, n)
        # (neither call wrote to the encoder: stream 0 and the last stream still hold what was set)
        assert np.array_equal(enc.get_state(native.STATE_MEM_MAIN, 0), main[STREAM0_ITEM])
        assert np.array_equal(enc.get_state(native.STATE_MEM_MAIN, S - 1), main[(n - 1) % P])
    finally:
        enc.close()


# ---- on a busy non-blocking side stream (tests/stream_probe.py) --------------------------------------------------------------

PAD = 4096      # sentinel bytes in front of and behind the probed output


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _probe_inputs(p, mode, n):
    """the batch's screens as probe inputs; the decoy is the same batch three items further round the pool"""
    main, aux, _ = pool()
    return p.input(main[_items(n)], main[_items(n, 3)]), p.input(aux[_items(n)], aux[_items(n, 3)])


def _palette_pair(p):
    pals = _palettes()
    return p.host(np.ascontiguousarray(pals["NTSC"], np.uint8).reshape(48), np.ascontiguousarray(pals["IIGS"], np.uint8).reshape(48))


@pytest.mark.parametrize("mode", MODES)
def test_render_rgb_on_a_busy_side_stream(native, mode):
    n = N_SECOND
    assert_trips(n)
    L = native.lib()
    p = Probe()
    dm, da = _probe_inputs(p, mode, n)
    out = p.output((PAD + n * FRAME + PAD,))
    pal = _palette_pair(p)

    def call(st):
        ok(native, L.iiv_render_rgb(mode, _hp(pal), n, native.dptr(dm), native.dptr(da), C.c_void_p(out.data_ptr() + PAD), st))
    call(native.stream_ptr())
    p.run(call)
    _check_every_frame(out[PAD:PAD + n * FRAME].view(n, 192, 560, 3), want_rgb(mode, "NTSC"))
    assert _all_hold(out[:PAD], SENTINEL_B) and _all_hold(out[PAD + n * FRAME:], SENTINEL_B)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_render_error_on_a_busy_side_stream(native, mode, width):
    """The zeroing memset of the call is stream work too: issued anywhere but on the caller's stream, sentinel B is added to."""
    import torch
    n = N_SECOND
    assert_trips(n)
    L = native.lib()
    refs = pool()[2][width]
    p = Probe()
    dm, da = _probe_inputs(p, mode, n)
    dr = p.input(refs[_items(n)], refs[_items(n, 3)])
    out = p.output((n + 2, 3, 3), torch.uint64)
    pal = _palette_pair(p)

    def call(st):
        ok(native, L.iiv_render_error(mode, _hp(pal), n, native.dptr(dm), native.dptr(da), native.dptr(dr), width,
                                      C.c_void_p(out.data_ptr() + 72), st))
    call(native.stream_ptr())
    p.run(call)
    got = Probe.bytes_of(out).cpu().numpy()
    _check_every_sum(got[72:72 + n * 72].view(np.uint64).reshape(n, 3, 3), want_sums(mode, width, "NTSC"), n)
    assert (got[:72] == SENTINEL_B).all() and (got[72 + n * 72:] == SENTINEL_B).all()
