"""GPU: the spatial filter (include/iivision.h section f16; csrc/iiv_filter.hip) against the numpy model (tests/spatial_model.py), byte
for byte: every height, width, frame count, clip count, tap pair and gain table of the grid on noise, a constant, a checkerboard and
single impulses at the corners, the edges and both sides of every tile seam; padded clip and frame strides; an out= tensor with other
strides; every refusal; and one call on a busy side stream."""
import ctypes as C

import numpy as np
import pytest

import spatial_cases as SC
import spatial_model as M
from device_guards import guarded, guards_kept, ok
from stream_cases import dp as _dp
from stream_probe import Probe

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _tables(pair, gain):
    tx, ty = (np.array(t, np.uint16) for t in (SC.TAP_PAIRS[pair] if isinstance(pair, int) else pair))
    g = np.ascontiguousarray(SC.GAINS[gain] if isinstance(gain, str) else gain, dtype=np.int16)
    return tx, ty, g


def _filter(native, src, out, c, n, H, W, pair, gain, st=None, strides=None):
    """the raw call on contiguous (c, n, H, W, 3) tensors, or with strides = (src clip, src frame, out clip, out frame)"""
    fb = H * W * 3
    s = strides or (n * fb, fb, n * fb, fb)
    tx, ty, g = _tables(pair, gain)
    return native.lib().iiv_filter_frames(c, n, H, W, _dp(src), s[0], s[1], _dp(out), s[2], s[3], native.hptr(tx), native.hptr(ty),
                                          native.hptr(g), st if st is not None else native.stream_ptr())


@pytest.mark.parametrize("W", SC.WIDTHS)
@pytest.mark.parametrize("H", SC.HEIGHTS)
def test_grid_equals_the_model(native, H, W):
    """every tap pair x gain x n_frames x n_clips of the grid on the block of nine frames; the output holds a sentinel before each
    call"""
    import torch
    block = torch.from_numpy(SC.block(H, W).copy()).cuda()
    for pair in range(len(SC.TAP_PAIRS)):
        for gain in SC.GAINS:
            want = SC.want(H, W, pair, gain)
            d_want = torch.from_numpy(want).cuda()              # (compared on the device; the host sees a mismatch only)
            for n in SC.N_FRAMES:
                for c in SC.N_CLIPS:
                    src = block[:c, :n].contiguous()
                    out = torch.full((c, n, H, W, 3), SC.SENTINEL, dtype=torch.uint8, device="cuda")
                    ok(native, _filter(native, src, out, c, n, H, W, pair, gain))
                    if not torch.equal(out, d_want[:c, :n]):
                        bad = np.argwhere(out.cpu().numpy() != want[:c, :n])
                        assert len(bad) == 0, "%d x %d, %d frames, %d clips, taps %d, gain %s: %d bytes differ, the first at %s" % (
                            H, W, n, c, pair, gain, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("H,W", [(SC.T_H + 1, 12), (2 * SC.T_H + 3, SC.T_W + 4)])
def test_padded_strides_and_guards(native, H, W):
    """clips and frames at padded strides in source and output (not the same ones), the padding holding a sentinel that must
    still be there; guard bytes around the output; the source read only"""
    import torch
    c, n, pair, gain = SC.CLIPS, SC.FRAMES, 2, "both"
    fb = H * W * 3
    sfs, scs = fb + 8, (fb + 8) * n + 24
    ofs, ocs = fb + 20, (fb + 20) * n + 4
    src = torch.full((c * scs,), 0x33, dtype=torch.uint8, device="cuda")
    src_view = torch.as_strided(src, (c, n, fb), (scs, sfs, 1))
    src_view.copy_(torch.from_numpy(SC.block(H, W).copy()).cuda().view(c, n, fb))
    buf, flat = guarded(c * ocs, 64, 64, GUARD)
    flat.fill_(SC.SENTINEL)
    ok(native, _filter(native, src, flat, c, n, H, W, pair, gain, strides=(scs, sfs, ocs, ofs)))
    want = SC.want(H, W, pair, gain)
    got = flat.cpu().numpy()
    owned = np.zeros(c * ocs, bool)
    for k in range(c):
        for t in range(n):
            at = k * ocs + t * ofs
            owned[at:at + fb] = True
            assert np.array_equal(got[at:at + fb], want[k, t].reshape(fb)), (k, t)
    assert (got[~owned] == SC.SENTINEL).all(), "the call wrote into the padding between frames or clips"
    assert guards_kept(buf, 64, c * ocs, GUARD)
    src_host, src_owned = src.cpu().numpy(), np.zeros(c * scs, bool)
    for k in range(c):
        for t in range(n):
            at = k * scs + t * sfs
            src_owned[at:at + fb] = True
            assert np.array_equal(src_host[at:at + fb], SC.block(H, W)[k, t].reshape(fb))
    assert (src_host[~src_owned] == 0x33).all()


def test_out_with_other_strides_through_the_binding(native):
    """frames a view with a padded frame stride and out= a view with a padded clip stride, one clip and several; by default a new
    contiguous tensor"""
    import torch
    H, W, pair, gain = SC.T_H + 1, 12, 3, "random"
    tx, ty = SC.TAP_PAIRS[pair]
    want = SC.want(H, W, pair, gain)
    block = torch.from_numpy(SC.block(H, W).copy()).cuda()
    wide = torch.full((SC.CLIPS, SC.FRAMES + 1, H, W, 3), 0x33, dtype=torch.uint8, device="cuda")
    frames = wide[:, :SC.FRAMES]
    frames.copy_(block)
    room = torch.full((SC.CLIPS, SC.FRAMES, 2, H, W, 3), SC.SENTINEL, dtype=torch.uint8, device="cuda")
    out = room[:, :, 1]
    assert native.filter_frames(frames, tx, ty, SC.GAINS[gain], out=out) is out
    assert np.array_equal(out.cpu().numpy(), want) and bool((room[:, :, 0] == SC.SENTINEL).all()) and bool((wide[:, SC.FRAMES] == 0x33).all())
    got = native.filter_frames(frames[1], list(tx), np.array(ty), SC.GAINS[gain].astype(np.int64))
    assert got.is_contiguous() and tuple(got.shape) == (SC.FRAMES, H, W, 3) and np.array_equal(got.cpu().numpy(), want[1])
    got = native.filter_frames(block, tx, ty, SC.GAINS[gain])
    assert got.data_ptr() != block.data_ptr() and np.array_equal(got.cpu().numpy(), want)


def test_refusals_write_nothing(native):
    import torch
    H, W, c, n, pair, gain = 5, 12, SC.CLIPS, SC.FRAMES, 2, "both"
    fb = H * W * 3
    src = torch.from_numpy(SC.block(H, W).copy()).cuda()
    out = torch.full((c, n, H, W, 3), SC.SENTINEL, dtype=torch.uint8, device="cuda")
    L, st, null = native.lib(), native.stream_ptr(), C.c_void_p(0)
    tx, ty, g = _tables(pair, gain)

    def off(t, k):
        return C.c_void_p(t.data_ptr() + k)

    def u16(*v):
        return np.array(v, np.uint16)

    def gain_with(at, value):
        a = g.copy()
        a[at] = value
        return a

    def call(c_=c, n_=n, h=H, w=W, s=_dp(src), scs=n * fb, sfs=fb, o=_dp(out), ocs=n * fb, ofs=fb, tx_=tx, ty_=ty, g_=g):
        return L.iiv_filter_frames(c_, n_, h, w, s, scs, sfs, o, ocs, ofs, native.hptr(tx_) if tx_ is not None else null,
                                   native.hptr(ty_) if ty_ is not None else null, native.hptr(g_) if g_ is not None else null, st)
    refused = [call(c_=-1), call(n_=-1), call(h=0), call(w=0), call(h=3, w=2), call(h=3, w=10), call(h=1, w=6),
               call(s=off(src, 1)), call(o=off(out, 2)), call(scs=n * fb + 2), call(sfs=fb + 1), call(ocs=n * fb + 3), call(ofs=fb + 2),
               call(sfs=fb - 4), call(ofs=fb - 4),
               call(h=-1, w=-4), call(h=2, w=2), call(h=2, w=6), call(h=2, w=30),
               call(tx_=None), call(ty_=None), call(g_=None),
               call(tx_=u16(0, 0, 257, 0, 0)), call(ty_=u16(16, 64, 96, 64, 15)), call(tx_=u16(16, 64, 96, 64, 17)),
               call(g_=gain_with(0, -257)), call(g_=gain_with(255, 1025)),
               call(o=_dp(src)), call(s=null), call(o=null)]
    assert refused == [native.ERR_INVALID] * len(refused)
    assert call(c_=0) == 0 and call(n_=0) == 0                      # no work: succeeds, writes nothing
    torch.cuda.synchronize()
    assert bool((out == SC.SENTINEL).all()) and np.array_equal(src.cpu().numpy(), SC.block(H, W))
    assert call() == 0
    assert np.array_equal(out.cpu().numpy(), SC.want(H, W, pair, gain))
    # the binding: every rule before the call
    good = (SC.TAP_PAIRS[pair][0], SC.TAP_PAIRS[pair][1], SC.GAINS[gain])
    fresh = torch.full((c, n, H, W, 3), SC.SENTINEL, dtype=torch.uint8, device="cuda")
    for at, bad in ((0, (16, 64, 96, 64, 15)), (1, (0, 0, 257, 0, 0)), (0, (1, 2, 3)), (2, np.full(256, 1025)), (2, np.zeros(255, np.int16))):
        args = list(good)
        args[at] = bad
        with pytest.raises(ValueError):
            native.filter_frames(src, *args, out=fresh)
    with pytest.raises(ValueError):
        native.filter_frames(src, *good, out=src)                                   # in place
    with pytest.raises(ValueError):
        native.filter_frames(src[:, 1:], *good, out=src[:, :2])                     # another part of the same storage
    with pytest.raises(ValueError):
        native.filter_frames(src, *good, out=fresh[:, :2])                          # another shape
    with pytest.raises(ValueError):
        native.filter_frames(src.view(c, n, H * W // 2, 2, 3), *good)               # two pixels wide
    with pytest.raises(ValueError):
        native.filter_frames(src.view(c, n, H * 2, W // 2, 3), *good)               # six pixels wide
    with pytest.raises(ValueError):
        native.filter_frames(src[..., :2], *good)                                   # not a frame of RGB pixels
    with pytest.raises(ValueError):
        native.filter_frames(src.cpu(), *good)
    torch.cuda.synchronize()
    assert bool((fresh == SC.SENTINEL).all()) and np.array_equal(src.cpu().numpy(), SC.block(H, W))


def test_on_a_busy_side_stream(native):
    """One call under the probe of tests/stream_probe.py: the source is a decoy until the side stream reaches the call, the output a
    sentinel; the taps and the gain are host arrays scribbled over right after the call returns"""
    H, W, c, n, pair, gain = 2 * SC.T_H + 3, SC.T_W + 4, SC.CLIPS, SC.FRAMES, 2, "both"
    fb = H * W * 3
    real = SC.block(H, W)
    decoy = np.random.default_rng(1609).integers(0, 256, real.shape).astype(np.uint8)
    p = Probe()
    src = p.input(real, decoy)
    out = p.output((c, n, H, W, 3))
    tx, ty, g = _tables(pair, gain)
    tx, ty, g = p.host(tx, tx[::-1]), p.host(ty, np.array(SC.ASYMMETRIC_TAPS)), p.host(g, np.zeros(256))

    def call(st):
        ok(native, native.lib().iiv_filter_frames(c, n, H, W, _dp(src), n * fb, fb, _dp(out), n * fb, fb, native.hptr(tx),
                                                  native.hptr(ty), native.hptr(g), st))
    call(native.stream_ptr())          # the warm-up, on the decoy
    p.run(call)
    assert np.array_equal(out.cpu().numpy(), SC.want(H, W, pair, gain))
    assert not np.array_equal(M.filter_frames(decoy, *SC.TAP_PAIRS[pair], SC.GAINS[gain]), SC.want(H, W, pair, gain))
