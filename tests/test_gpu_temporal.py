"""GPU: the temporal hold (include/iivision.h section f14; csrc/iiv_temporal.hip) against the numpy model (tests/temporal_model.py),
byte for byte, counts included: every pixel count, frame count, clip count and (lo, hi) of the grid on four kinds of input, padded
clip and frame strides, in place, a clip continued over two and three calls, d_counts NULL, every refusal, and one call on a busy
side stream."""
import ctypes as C

import numpy as np
import pytest

import temporal_cases as TC
from device_guards import guarded, guards_kept, ok
from stream_cases import dp as _dp
from stream_probe import Probe

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _hold(native, src, out, state, first, pair, counts, c, n, pixels, st=None, strides=None):
    """the raw call on contiguous (c, n, pixels, 3) tensors, or with strides = (src clip, src frame, out clip, out frame)"""
    fb = pixels * 3
    s = strides or (n * fb, fb, n * fb, fb)
    return native.lib().iiv_temporal_hold(c, n, pixels, _dp(src), s[0], s[1], _dp(out), s[2], s[3], _dp(state), fb, 1 if first else 0,
                                          pair[0], pair[1], _dp(counts), st if st is not None else native.stream_ptr())


@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("pixels", TC.PIXELS)
def test_grid_equals_the_model(native, pixels, kind):
    """every n_frames x n_clips x (lo, hi) of the grid: output, state and counts; the tensors hold a sentinel before each call"""
    import torch
    block = torch.from_numpy(TC.clip(kind, pixels).copy()).cuda()
    for pair in TC.PAIRS:
        want, want_counts = TC.want(kind, pixels, pair)
        d_want = torch.from_numpy(want.copy()).cuda()              # (compared on the device; the host sees a mismatch only)
        d_want_counts = torch.from_numpy(want_counts.view(np.int32).copy()).cuda()
        for n in TC.N_FRAMES:
            for c in TC.N_CLIPS:
                src = block[:c, :n].contiguous()
                out = torch.full((c, n, pixels, 3), TC.SENTINEL, dtype=torch.uint8, device="cuda")
                state = torch.full((c, pixels, 3), TC.SENTINEL, dtype=torch.uint8, device="cuda")
                counts = torch.full((c, n, 3), 0x5B5B5B5B, dtype=torch.int32, device="cuda")
                ok(native, _hold(native, src, out, state, True, pair, counts, c, n, pixels))
                label = "%s, %d pixels, %d frames, %d clips, %s" % (kind, pixels, n, c, pair)
                if not torch.equal(out, d_want[:c, :n]):
                    bad = np.argwhere(out.cpu().numpy() != want[:c, :n])
                    assert len(bad) == 0, "%s: %d bytes differ, the first at %s" % (label, len(bad), bad[:4].tolist())
                assert torch.equal(state, d_want[:c, n - 1]), label
                assert torch.equal(counts, d_want_counts[:c, :n]), "%s: counts %s, model %s" % (
                    label, counts.cpu().numpy().view(np.uint32).tolist(), want_counts[:c, :n].tolist())


@pytest.mark.parametrize("pixels", (260, 53760))
def test_padded_strides_and_guards(native, pixels):
    """clips and frames at padded strides in source and output (not the same ones), the padding holding a sentinel that must
    still be there; guard bytes around the output, the state and the counts"""
    import torch
    c, n, pair, kind = 3, TC.RING + 1, (3, 12), "near"
    fb = pixels * 3
    sfs, scs = fb + 8, (fb + 8) * n + 24
    ofs, ocs = fb + 20, (fb + 20) * n + 4
    src = torch.full((c * scs,), 0x33, dtype=torch.uint8, device="cuda")
    clip = torch.from_numpy(TC.clip(kind, pixels)[:c, :n].copy()).cuda()
    src_view = torch.as_strided(src, (c, n, fb), (scs, sfs, 1))
    src_view.copy_(clip.view(c, n, fb))
    buf, flat = guarded(c * ocs, 64, 64, GUARD)
    flat.fill_(TC.SENTINEL)
    sbuf, state = guarded(c * fb, 64, 64, GUARD)
    cbuf, cflat = guarded(c * n * 12, 64, 64, GUARD)
    ok(native, _hold(native, src, flat, state, True, pair, cflat, c, n, pixels, strides=(scs, sfs, ocs, ofs)))
    want, want_counts = TC.want(kind, pixels, pair)
    got = flat.cpu().numpy()
    owned = np.zeros(c * ocs, bool)
    for k in range(c):
        for t in range(n):
            at = k * ocs + t * ofs
            owned[at:at + fb] = True
            assert np.array_equal(got[at:at + fb], want[k, t].reshape(fb)), (k, t)
    assert (got[~owned] == TC.SENTINEL).all(), "the call wrote into the padding between frames or clips"
    assert np.array_equal(state.cpu().numpy().reshape(c, pixels, 3), want[:c, n - 1])
    assert np.array_equal(cflat.cpu().numpy().view(np.uint32).reshape(c, n, 3), want_counts[:c, :n])
    assert guards_kept(buf, 64, c * ocs, GUARD) and guards_kept(sbuf, 64, c * fb, GUARD) and guards_kept(cbuf, 64, c * n * 12, GUARD)
    # the source is read only, its padding included
    assert np.array_equal(src_view.cpu().numpy().reshape(c, n, pixels, 3), TC.clip(kind, pixels)[:c, :n])
    src_host, src_owned = src.cpu().numpy(), np.zeros(c * scs, bool)
    for k in range(c):
        for t in range(n):
            src_owned[k * scs + t * sfs:k * scs + t * sfs + fb] = True
    assert (src_host[~src_owned] == 0x33).all() and int((~src_owned).sum()) == c * scs - c * n * fb


@pytest.mark.parametrize("kind,pair", [("near", (3, 12)), ("flip", (0, 255)), ("ramp", (4, 4))])
def test_in_place(native, kind, pair):
    """d_out == d_src with equal strides, past two turns of the ring, through the binding as well"""
    import torch
    pixels, c, n = 1028, 3, 2 * TC.RING + 1
    want, want_counts = TC.want(kind, pixels, pair)
    data = torch.from_numpy(TC.clip(kind, pixels).copy()).cuda()
    state = torch.empty((c, pixels, 3), dtype=torch.uint8, device="cuda")
    counts = torch.empty((c, n, 3), dtype=torch.int32, device="cuda")
    ok(native, _hold(native, data, data, state, True, pair, counts, c, n, pixels))
    assert np.array_equal(data.cpu().numpy(), want) and np.array_equal(state.cpu().numpy(), want[:, n - 1])
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want_counts)
    frames = torch.from_numpy(TC.clip(kind, pixels).copy()).cuda().view(c, n, 257, 4, 3)
    out, st, cn = native.temporal_hold(frames, pair[0], pair[1], out=frames, counts=True)
    assert out.data_ptr() == frames.data_ptr() and tuple(st.shape) == (c, 257, 4, 3) and tuple(cn.shape) == (c, n, 3)
    assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)
    assert np.array_equal(cn.cpu().numpy().view(np.uint32), want_counts)


@pytest.mark.parametrize("cuts", [(1,), (TC.RING,), (3, TC.RING + 2), (1, 2)])
@pytest.mark.parametrize("pair", [(3, 12), (16, 64)])
def test_continuation_over_two_and_three_calls(native, pair, cuts):
    """the state an earlier call left continues the clip: the pieces equal one call's frames, counts and final state; the
    binding's state=None / state=<returned> does the same on one clip of another shape"""
    import torch
    pixels, c, n, kind = 252, 3, 2 * TC.RING + 1, "near"
    want, want_counts = TC.want(kind, pixels, pair)
    block = torch.from_numpy(TC.clip(kind, pixels).copy()).cuda()
    state = torch.full((c, pixels, 3), TC.SENTINEL, dtype=torch.uint8, device="cuda")
    edges = (0,) + cuts + (n,)
    for a, b in zip(edges[:-1], edges[1:]):
        src = block[:, a:b].contiguous()
        out = torch.full((c, b - a, pixels, 3), TC.SENTINEL, dtype=torch.uint8, device="cuda")
        counts = torch.empty((c, b - a, 3), dtype=torch.int32, device="cuda")
        ok(native, _hold(native, src, out, state, a == 0, pair, counts, c, b - a, pixels))
        assert np.array_equal(out.cpu().numpy(), want[:, a:b]), (a, b)
        assert np.array_equal(counts.cpu().numpy().view(np.uint32), want_counts[:, a:b]), (a, b)
        assert np.array_equal(state.cpu().numpy(), want[:, b - 1]), (a, b)
    st = None
    for a, b in zip(edges[:-1], edges[1:]):
        frames = block[1, a:b].view(b - a, 9, 28, 3)          # one clip, a view with the clip's own frame stride
        out, st, cn = native.temporal_hold(frames, pair[0], pair[1], state=st, counts=True)
        assert tuple(out.shape) == (b - a, 9, 28, 3) and tuple(st.shape) == (9, 28, 3) and tuple(cn.shape) == (b - a, 3)
        assert np.array_equal(out.cpu().numpy().reshape(b - a, pixels, 3), want[1, a:b])
        assert np.array_equal(cn.cpu().numpy().view(np.uint32), want_counts[1, a:b])
    assert np.array_equal(st.cpu().numpy().reshape(pixels, 3), want[1, n - 1])


def test_counts_may_be_null(native):
    import torch
    pixels, c, n, kind, pair = 1028, 3, TC.RING + 1, "noise", (16, 64)
    want, _ = TC.want(kind, pixels, pair)
    src = torch.from_numpy(TC.clip(kind, pixels)[:c, :n].copy()).cuda()
    out = torch.full((c, n, pixels, 3), TC.SENTINEL, dtype=torch.uint8, device="cuda")
    state = torch.empty((c, pixels, 3), dtype=torch.uint8, device="cuda")
    ok(native, _hold(native, src, out, state, True, pair, None, c, n, pixels))
    assert np.array_equal(out.cpu().numpy(), want[:c, :n]) and np.array_equal(state.cpu().numpy(), want[:c, n - 1])
    got, st = native.temporal_hold(src.view(c, n, 257, 4, 3), *pair)
    assert np.array_equal(got.cpu().numpy().reshape(c, n, pixels, 3), want[:c, :n])


def test_refusals_write_nothing(native):
    import torch
    pixels, c, n, kind, pair = 260, 3, 3, "near", (3, 12)
    fb = pixels * 3
    src = torch.from_numpy(TC.clip(kind, pixels)[:c, :n].copy()).cuda()
    out = torch.full((c, n, pixels, 3), TC.SENTINEL, dtype=torch.uint8, device="cuda")
    state = torch.full((c, pixels, 3), TC.SENTINEL, dtype=torch.uint8, device="cuda")
    counts = torch.full((c, n, 3), 0x5B5B5B5B, dtype=torch.int32, device="cuda")
    L, st, null = native.lib(), native.stream_ptr(), C.c_void_p(0)

    def off(t, k):
        return C.c_void_p(t.data_ptr() + k)

    def call(c_=c, n_=n, px=pixels, s=_dp(src), scs=n * fb, sfs=fb, o=_dp(out), ocs=n * fb, ofs=fb, h=_dp(state), ss=fb, first=1,
             lo=pair[0], hi=pair[1], cn=_dp(counts)):
        return L.iiv_temporal_hold(c_, n_, px, s, scs, sfs, o, ocs, ofs, h, ss, first, lo, hi, cn, st)
    refused = [call(c_=-1), call(n_=-1), call(px=0), call(px=-4), call(px=258), call(px=261),
               call(s=off(src, 1)), call(o=off(out, 2)), call(h=off(state, 3)), call(cn=off(counts, 2)),
               call(scs=n * fb + 2), call(sfs=fb + 1), call(ocs=n * fb + 3), call(ofs=fb + 2), call(ss=fb + 2),
               call(sfs=fb - 4), call(ofs=fb - 4), call(ss=fb - 4),
               call(lo=-1), call(hi=256), call(lo=13), call(lo=256, hi=256),
               call(s=null), call(o=null), call(h=null)]
    assert refused == [native.ERR_INVALID] * len(refused)
    assert call(c_=0) == 0 and call(n_=0) == 0                      # no work: succeeds, writes nothing
    torch.cuda.synchronize()
    assert bool((out == TC.SENTINEL).all()) and bool((state == TC.SENTINEL).all()) and bool((counts == 0x5B5B5B5B).all())
    assert call() == 0
    want, want_counts = TC.want(kind, pixels, pair)
    assert np.array_equal(out.cpu().numpy(), want[:c, :n])
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want_counts[:c, :n])
    frames = src.view(c, n, 65, 4, 3)
    for bad in ((13, 12), (-1, 4), (0, 256)):
        with pytest.raises(ValueError):
            native.temporal_hold(frames, *bad)
    with pytest.raises(ValueError):
        native.temporal_hold(frames, 3, 12, state=state)                      # (3, 260, 3) is not (3, 65, 4, 3)
    with pytest.raises(ValueError):
        native.temporal_hold(frames, 3, 12, out=out)                          # another shape
    with pytest.raises(ValueError):
        native.temporal_hold(src.view(c, n, 260, 3)[:, :, :, :2], 3, 12)       # not a frame of RGB pixels
    with pytest.raises(ValueError):
        native.temporal_hold(src.view(c, n, 65, 4, 3)[:, :, :, :3], 3, 12)     # 195 pixels, and rows that are not dense


def test_on_a_busy_side_stream(native):
    """One continuing call under the probe of tests/stream_probe.py: source and state are decoys until the side stream reaches
    the call; output and counts hold a sentinel, so a clearing of the counts issued on another stream is overwritten."""
    import torch
    pixels, c, n, pair, kind = 1028, 3, TC.RING + 1, (3, 12), "near"
    block = TC.clip(kind, pixels)
    want, want_counts = TC.want(kind, pixels, pair)
    real, decoy = block[:c, 3:3 + n], TC.clip("noise", pixels)[:c, :n]
    state_real = torch.from_numpy(want[:c, 2].copy()).cuda()                 # the state behind frames 0..2
    state_decoy = torch.from_numpy(TC.clip("noise", pixels)[:c, n].copy()).cuda()
    p = Probe()
    src = p.input(real, decoy)
    state, kept = p.in_place(state_real, state_decoy)
    out = p.output((c, n, pixels, 3))
    counts = p.output((c, n, 3), torch.int32)

    def call(st):
        ok(native, _hold(native, src, out, state, False, pair, counts, c, n, pixels, st=st))
    call(native.stream_ptr())          # the warm-up, on the decoys
    p.run(call)
    assert np.array_equal(out.cpu().numpy(), want[:c, 3:3 + n])
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want_counts[:c, 3:3 + n])
    assert np.array_equal(kept.cpu().numpy(), want[:c, 2 + n])
