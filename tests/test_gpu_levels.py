"""GPU: picture levels (include/iivision.h section f15; csrc/iiv_levels.hip) against the numpy model (tests/levels_model.py), count
for count and byte for byte: every pixel count, frame count and clip count of the grid on five kinds of input -- a flat frame and
two alternating values among them, where the histogram's wave-level pre-combine does all or half of the counting --, the tables
that reach both clamps, per-clip tables against stride 0, frame counts around a range of frames, padded clip and frame strides,
in place, every refusal, and one call of each kernel on a busy side stream."""
import ctypes as C

import numpy as np
import pytest

import levels_cases as LC
import levels_model as M
from device_guards import guarded, guards_kept, ok
from stream_cases import dp as _dp
from stream_probe import Probe

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _hist(native, src, hist, c, n, pixels, st=None, strides=None):
    fb = pixels * 3
    s = strides or (n * fb, fb)
    return native.lib().iiv_levels_histogram(c, n, pixels, _dp(src), s[0], s[1], _dp(hist), st if st is not None else native.stream_ptr())


def _apply(native, src, out, lut, m, c, n, pixels, st=None, strides=None, table_strides=(768, 20)):
    fb = pixels * 3
    s = strides or (n * fb, fb, n * fb, fb)
    return native.lib().iiv_levels_apply(c, n, pixels, _dp(src), s[0], s[1], _dp(out), s[2], s[3], _dp(lut), table_strides[0], _dp(m),
                                         table_strides[1], st if st is not None else native.stream_ptr())


@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("pixels", LC.PIXELS)
def test_histogram_grid_equals_the_model(native, pixels, kind):
    """every n_frames x n_clips of the grid: all 1024 counts of every frame; the output holds a sentinel before each call"""
    import torch
    block = torch.from_numpy(LC.clip(kind, pixels).copy()).cuda()
    want = LC.want_hist(kind, pixels)
    d_want = torch.from_numpy(want.view(np.int32).copy()).cuda()
    for n in LC.N_FRAMES:
        for c in LC.N_CLIPS:
            src = block[:c, :n].contiguous()
            hist = torch.full((c, n, 4, 256), 0x5B5B5B5B, dtype=torch.int32, device="cuda")
            ok(native, _hist(native, src, hist, c, n, pixels))
            label = "%s, %d pixels, %d frames, %d clips" % (kind, pixels, n, c)
            if not torch.equal(hist, d_want[:c, :n]):
                bad = np.argwhere(hist.cpu().numpy().view(np.uint32) != want[:c, :n])
                assert len(bad) == 0, "%s: %d counts differ, the first at %s" % (label, len(bad), bad[:4].tolist())
            assert bool((hist.long().sum(dim=-1) == pixels).all()), label
    # the binding, on a view with the clip's own strides
    got = native.levels_histogram(block[:, 1:3].view(LC.CLIPS, 2, pixels // 4, 4, 3))
    assert tuple(got.shape) == (LC.CLIPS, 2, 4, 256) and torch.equal(got, d_want[:, 1:3])
    one = native.levels_histogram(block[1].view(LC.FRAMES, 1, pixels, 3))
    assert tuple(one.shape) == (LC.FRAMES, 4, 256) and torch.equal(one, d_want[1])


@pytest.mark.parametrize("name", LC.TABLES)
@pytest.mark.parametrize("pixels", LC.PIXELS)
def test_apply_grid_equals_the_model(native, pixels, name):
    """every n_frames x n_clips of the grid with a table and a matrix per clip; with stride 0 every clip gets clip 0's"""
    import torch
    kind = "extremes" if name in ("max", "min") and pixels == 260 else "noise"
    block = torch.from_numpy(LC.clip(kind, pixels).copy()).cuda()
    want = LC.want_apply(kind, pixels, name)
    d_want = torch.from_numpy(want.copy()).cuda()
    lut, m = LC.tables(name)
    d_lut, d_m = LC.device_tables(torch, lut, m)
    for n in LC.N_FRAMES:
        for c in LC.N_CLIPS:
            src = block[:c, :n].contiguous()
            out = torch.full((c, n, pixels, 3), LC.SENTINEL, dtype=torch.uint8, device="cuda")
            ok(native, _apply(native, src, out, d_lut, d_m, c, n, pixels))
            label = "%s, %d pixels, %d frames, %d clips" % (name, pixels, n, c)
            if not torch.equal(out, d_want[:c, :n]):
                bad = np.argwhere(out.cpu().numpy() != want[:c, :n])
                assert len(bad) == 0, "%s: %d bytes differ, the first at %s" % (label, len(bad), bad[:4].tolist())
    if name in ("random", "small"):
        # stride 0 for one or both: every clip through clip 0's table and / or matrix
        src = block[:, :2].contiguous()
        for ls, ms in ((0, 0), (0, 20), (768, 0)):
            out = torch.full((LC.CLIPS, 2, pixels, 3), LC.SENTINEL, dtype=torch.uint8, device="cuda")
            ok(native, _apply(native, src, out, d_lut, d_m, LC.CLIPS, 2, pixels, table_strides=(ls, ms)))
            shared = M.apply_clips(LC.clip(kind, pixels)[:, :2], lut if ls else lut[[0, 0, 0]], m if ms else m[[0, 0, 0]])
            assert np.array_equal(out.cpu().numpy(), shared), (name, pixels, ls, ms)
            assert ls and ms or not np.array_equal(shared, want[:, :2])
        # the binding: per-clip tables, one pair for all clips, one table for the three channels
        frames = block.view(LC.CLIPS, LC.FRAMES, pixels // 4, 4, 3)
        assert torch.equal(native.levels_apply(frames, lut, m).view(want.shape), d_want)
        got = native.levels_apply(frames[1], lut[0, 2], m[2])
        assert np.array_equal(got.cpu().numpy().reshape(LC.FRAMES, pixels, 3), M.apply(LC.clip(kind, pixels)[1], lut[0, 2], m[2]))


def test_the_identity_and_the_saturations(native):
    """the identity table with 256 * I returns the bytes; saturation 0 is grey, 256 the identity, 1024 clamps on both sides"""
    import frame_grabber
    import torch
    x = LC.clip("noise", 1028)
    frames = torch.from_numpy(x.copy()).cuda().view(LC.CLIPS, LC.FRAMES, 257, 4, 3)
    assert torch.equal(native.levels_apply(frames, M.IDENTITY_LUT), frames)
    assert torch.equal(native.levels_apply(frames, M.IDENTITY_LUT, frame_grabber.saturation_matrix(256)), frames)
    grey = native.levels_apply(frames, M.IDENTITY_LUT, frame_grabber.saturation_matrix(0)).cpu().numpy().reshape(x.shape)
    assert (grey == M.luma(x)[..., None]).all()
    vivid = native.levels_apply(frames, M.IDENTITY_LUT, frame_grabber.saturation_matrix(1024)).cpu().numpy().reshape(x.shape)
    assert np.array_equal(vivid, M.apply(x, M.IDENTITY_LUT, M.saturation_matrix(1024))) and (vivid == 0).any() and (vivid == 255).any()
    lut = frame_grabber.levels_lut(16, 235, gamma=2.2, brightness=-5, contrast=1.2)
    got = native.levels_apply(frames, lut, frame_grabber.saturation_matrix(400)).cpu().numpy().reshape(x.shape)
    assert np.array_equal(got, M.apply(x, M.levels_lut(16, 235, 2.2, -5, 1.2), M.saturation_matrix(400)))


@pytest.mark.parametrize("pixels", (8, 1028))
def test_apply_over_ranges_of_frames(native, pixels):
    """frame counts around kLevelsApplyFrames: a clip is cut into ranges of frames, each an item of its own"""
    import torch
    x = LC.clip("noise", pixels, LC.RANGE_FRAMES)
    lut, m = LC.tables("small")
    want = M.apply_clips(x, lut, m)
    d_lut, d_m = LC.device_tables(torch, lut, m)
    block = torch.from_numpy(x.copy()).cuda()
    for n in (LC.APPLY_FRAMES - 1, LC.APPLY_FRAMES, LC.APPLY_FRAMES + 1, 2 * LC.APPLY_FRAMES, LC.RANGE_FRAMES):
        src = block[:, :n].contiguous()
        out = torch.full((LC.CLIPS, n, pixels, 3), LC.SENTINEL, dtype=torch.uint8, device="cuda")
        ok(native, _apply(native, src, out, d_lut, d_m, LC.CLIPS, n, pixels))
        assert np.array_equal(out.cpu().numpy(), want[:, :n]), n
    hist = native.levels_histogram(block.view(LC.CLIPS, LC.RANGE_FRAMES, pixels // 4, 4, 3))
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), M.histogram(x))


@pytest.mark.parametrize("pixels", (260, 53760))
def test_padded_strides_and_guards(native, pixels):
    """clips and frames at padded strides in source and output (not the same ones), the padding holding a sentinel that must
    still be there; guard bytes around both outputs; tables at padded strides too"""
    import torch
    c, n, kind = 3, LC.APPLY_FRAMES + 1, "noise"
    x = LC.clip(kind, pixels, LC.RANGE_FRAMES)[:, :n]
    fb = pixels * 3
    sfs, scs = fb + 8, (fb + 8) * n + 24
    ofs, ocs = fb + 20, (fb + 20) * n + 4
    src = torch.full((c * scs,), 0x33, dtype=torch.uint8, device="cuda")
    src_view = torch.as_strided(src, (c, n, fb), (scs, sfs, 1))
    src_view.copy_(torch.from_numpy(x.copy()).cuda().view(c, n, fb))
    lut, m = LC.tables("small")
    ls, ms = 768 + 12, 24
    d_lut = torch.full((c, ls), 0x77, dtype=torch.uint8, device="cuda")
    d_lut[:, :768] = torch.from_numpy(lut.reshape(c, 768).copy()).cuda()
    d_m = torch.full((c, ms // 2), 0x7777, dtype=torch.int16, device="cuda")
    d_m[:, :9] = torch.from_numpy(m.reshape(c, 9).astype(np.int16)).cuda()
    buf, flat = guarded(c * ocs, 64, 64, GUARD)
    flat.fill_(LC.SENTINEL)
    hbuf, hflat = guarded(c * n * 4096, 64, 64, GUARD)
    ok(native, _hist(native, src, hflat, c, n, pixels, strides=(scs, sfs)))
    ok(native, _apply(native, src, flat, d_lut, d_m, c, n, pixels, strides=(scs, sfs, ocs, ofs), table_strides=(ls, ms)))
    want = M.apply_clips(x, lut, m)
    got = flat.cpu().numpy()
    owned = np.zeros(c * ocs, bool)
    for k in range(c):
        for t in range(n):
            at = k * ocs + t * ofs
            owned[at:at + fb] = True
            assert np.array_equal(got[at:at + fb], want[k, t].reshape(fb)), (k, t)
    assert (got[~owned] == LC.SENTINEL).all(), "the call wrote into the padding between frames or clips"
    assert np.array_equal(hflat.cpu().numpy().view(np.uint32).reshape(c, n, 4, 256), M.histogram(x))
    assert guards_kept(buf, 64, c * ocs, GUARD) and guards_kept(hbuf, 64, c * n * 4096, GUARD)
    # the source is read only, its padding included
    src_host, src_owned = src.cpu().numpy(), np.zeros(c * scs, bool)
    for k in range(c):
        for t in range(n):
            src_owned[k * scs + t * sfs:k * scs + t * sfs + fb] = True
            assert np.array_equal(src_host[k * scs + t * sfs:k * scs + t * sfs + fb], x[k, t].reshape(fb))
    assert (src_host[~src_owned] == 0x33).all()


@pytest.mark.parametrize("name", ["small", "min", "sat1024"])
def test_in_place(native, name):
    """d_out == d_src with equal strides, over more than one range of frames, through the binding as well"""
    import torch
    pixels, c, n = 1028, 3, LC.RANGE_FRAMES
    x = LC.clip("noise", pixels, n)
    lut, m = LC.tables(name)
    want = M.apply_clips(x, lut, m)
    d_lut, d_m = LC.device_tables(torch, lut, m)
    data = torch.from_numpy(x.copy()).cuda()
    ok(native, _apply(native, data, data, d_lut, d_m, c, n, pixels))
    assert np.array_equal(data.cpu().numpy(), want)
    frames = torch.from_numpy(x.copy()).cuda().view(c, n, 257, 4, 3)
    out = native.levels_apply(frames, lut, m, out=frames)
    assert out.data_ptr() == frames.data_ptr() and np.array_equal(out.cpu().numpy().reshape(want.shape), want)


def test_refusals_write_nothing(native):
    import torch
    pixels, c, n = 260, 3, 3
    fb = pixels * 3
    x = LC.clip("noise", pixels)
    src = torch.from_numpy(x.copy()).cuda()
    out = torch.full((c, n, pixels, 3), LC.SENTINEL, dtype=torch.uint8, device="cuda")
    hist = torch.full((c, n, 4, 256), 0x5B5B5B5B, dtype=torch.int32, device="cuda")
    lut, m = LC.tables("small")
    d_lut, d_m = LC.device_tables(torch, lut, m)
    L, st, null = native.lib(), native.stream_ptr(), C.c_void_p(0)

    def off(t, k):
        return C.c_void_p(t.data_ptr() + k)

    def hcall(c_=c, n_=n, px=pixels, s=_dp(src), scs=n * fb, sfs=fb, h=_dp(hist)):
        return L.iiv_levels_histogram(c_, n_, px, s, scs, sfs, h, st)

    def acall(c_=c, n_=n, px=pixels, s=_dp(src), scs=n * fb, sfs=fb, o=_dp(out), ocs=n * fb, ofs=fb, t=_dp(d_lut), ls=768, mm=_dp(d_m), ms=20):
        return L.iiv_levels_apply(c_, n_, px, s, scs, sfs, o, ocs, ofs, t, ls, mm, ms, st)
    refused = [hcall(c_=-1), hcall(n_=-1), hcall(px=0), hcall(px=-4), hcall(px=258), hcall(px=261), hcall(px=2 ** 31 + 4, sfs=3 * 2 ** 31 + 12),
               hcall(s=off(src, 1)), hcall(h=off(hist, 2)), hcall(scs=n * fb + 2), hcall(sfs=fb + 1), hcall(sfs=fb - 4), hcall(s=null), hcall(h=null),
               acall(c_=-1), acall(n_=-1), acall(px=0), acall(px=-4), acall(px=258), acall(px=261),
               acall(px=2 ** 40 + 4, sfs=3 * 2 ** 40 + 12, ofs=3 * 2 ** 40 + 12),
               acall(s=off(src, 1)), acall(o=off(out, 2)), acall(t=off(d_lut, 1)), acall(mm=off(d_m, 2)),
               acall(scs=n * fb + 2), acall(sfs=fb + 1), acall(ocs=n * fb + 3), acall(ofs=fb + 2), acall(ls=770), acall(ms=22),
               acall(sfs=fb - 4), acall(ofs=fb - 4), acall(ls=764), acall(ls=4), acall(ms=16), acall(ms=4),
               acall(s=null), acall(o=null), acall(t=null), acall(mm=null)]
    assert refused == [native.ERR_INVALID] * len(refused)
    assert hcall(c_=0) == 0 and hcall(n_=0) == 0 and acall(c_=0) == 0 and acall(n_=0) == 0       # no work: succeeds, writes nothing
    torch.cuda.synchronize()
    assert bool((out == LC.SENTINEL).all()) and bool((hist == 0x5B5B5B5B).all())
    assert hcall() == 0 and acall() == 0
    assert np.array_equal(out.cpu().numpy(), LC.want_apply("noise", pixels, "small"))
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), LC.want_hist("noise", pixels))
    frames = src.view(c, n, 65, 4, 3)
    with pytest.raises(ValueError):
        native.levels_apply(frames, M.IDENTITY_LUT, np.full((3, 3), 2048))               # outside Q8 +-8.0: refused before upload
    with pytest.raises(ValueError):
        native.levels_apply(frames, M.IDENTITY_LUT, out=out)                              # another shape
    with pytest.raises(ValueError):
        native.levels_apply(frames, lut[:2])
    for call in (native.levels_histogram, lambda f: native.levels_apply(f, M.IDENTITY_LUT)):
        with pytest.raises(ValueError):
            call(src.view(c, n, 260, 3)[:, :, :, :2])                                     # not a frame of RGB pixels
        with pytest.raises(ValueError):
            call(src.view(c, n, 65, 4, 3)[:, :, :, :3])                                   # 195 pixels, and rows that are not dense
        with pytest.raises(ValueError):
            call(x)                                                                       # a host array


def test_on_a_busy_side_stream(native):
    """One call of each kernel under the probe of tests/stream_probe.py: source and tables are decoys until the side stream
    reaches the calls; the outputs hold a sentinel, so anything issued on another stream is overwritten or reads the decoy."""
    import torch
    pixels, c, n = 1028, 3, 3
    real, decoy = LC.clip("noise", pixels), LC.clip("ramp", pixels)
    lut, m = LC.tables("small")
    lut_decoy, m_decoy = LC.tables("random")
    padded = lambda a: np.concatenate([a.reshape(c, 9), np.zeros((c, 1), a.dtype)], axis=1).astype(np.int16)     # noqa: E731
    p = Probe()
    src = p.input(real, decoy)
    d_lut = p.input(lut, lut_decoy)
    d_m = p.input(padded(m), padded(m_decoy))
    out = p.output((c, n, pixels, 3))
    hist = p.output((c, n, 4, 256), torch.int32)

    def call(st):
        ok(native, _hist(native, src, hist, c, n, pixels, st=st))
        ok(native, _apply(native, src, out, d_lut, d_m, c, n, pixels, st=st))
    call(native.stream_ptr())          # the warm-up, on the decoys
    p.run(call)
    assert np.array_equal(out.cpu().numpy(), LC.want_apply("noise", pixels, "small"))
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), LC.want_hist("noise", pixels))
