"""GPU: csrc/iiv_ingest.hip where its design takes its risks -- byte for byte against the oracle, which
tests/test_ingest_model.py holds to an independent model of the contract on the CPU.
  palettes       exact ties, duplicate colours, coefficient extremes and one-step neighbours (ingest_model.PALETTES): the
                 kernels' arg-min of linear forms and the tie rules in the keys' low bits
  frame counts   partly filled waves of the error-diffusion kernel (six frame slots per workgroup), nothing written behind
                 the last frame
  source offsets a batch that starts 4, 8, 12, .. bytes into its allocation: the aligned-dword loads and the 64-byte blocks
                 of the LDS-DMA stream
  output offsets out= views at the 8-byte alignment the contract asks for
  refusals       a source or an output below its alignment is an IIVError and writes nothing"""

import numpy as np
import pytest

from device_guards import guarded, guards_kept
import ingest_model as M
from ingest_model import NAMES, frames_of, palette

MODES = [M.DHGR, M.HGR]
FRAME_BYTES = 192 * 280 * 3
GUARD = 0xEE


def _expected(O, mode, pal, frames, dither):
    main = np.empty((len(frames), 32, 256), np.uint8)
    aux = np.empty((len(frames), 32, 256), np.uint8) if mode == M.DHGR else None
    for i in range(len(frames)):
        m, a = O.frame_to_memory_map(mode, pal, frames[i], dither)
        main[i] = m
        if aux is not None:
            aux[i] = a
    return main, aux


def _different_frames():
    """thirteen frames, no two alike: picture-like content and noise by turns"""
    rng = np.random.default_rng(77)
    y, x = np.mgrid[0:192, 0:280]
    out = np.empty((13, 192, 280, 3), np.uint8)
    for i in range(13):
        if i % 2:
            out[i] = rng.integers(0, 256, (192, 280, 3))
        else:
            out[i] = np.stack([(x + 19 * i) * 255 // 526, (y * (i + 2)) % 256, (x * 3 + y * 5 + 31 * i) % 256], axis=-1)
    return out


_cache = {}


def _batch(O, mode, dither):
    """(frames, expected main, expected aux) of the thirteen frames under the NTSC palette: computed once per mode and dither"""
    if "frames" not in _cache:
        _cache["frames"] = _different_frames()
    key = (mode, dither)
    if key not in _cache:
        _cache[key] = _expected(O, mode, O.PALETTE_RGB[5], _cache["frames"], dither)
    return (_cache["frames"],) + _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_palettes(native, O, name, mode):
    import torch
    pal, frames = palette(O, name), frames_of(O, name)
    dev = torch.from_numpy(frames).cuda()
    for dither in M.DITHERS_GPU:
        main, aux = native.frames_to_memory_maps(mode, pal, dev, dither)
        em, ea = _expected(O, mode, pal, frames, dither)
        main = main.cpu().numpy()
        for i in range(len(frames)):
            assert (main[i] == em[i]).all(), (name, mode, dither, M.FRAME_KINDS[i], int((main[i] != em[i]).sum()))
        if mode == M.DHGR:
            aux = aux.cpu().numpy()
            for i in range(len(frames)):
                assert (aux[i] == ea[i]).all(), (name, mode, dither, M.FRAME_KINDS[i], "aux", int((aux[i] != ea[i]).sum()))
        else:
            assert aux is None


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dither,n", [(M.DITHER_DIFFUSION, n) for n in (1, 2, 3, 4, 5, 6, 7, 13)] + [(32, n) for n in (1, 2, 7)])
def test_frame_counts(native, O, mode, dither, n):
    """n different frames into buffers of n + 1: frames 0 .. n - 1 are the oracle's (holes zero), frame n keeps its fill."""
    import torch
    frames, em, ea = _batch(O, mode, dither)
    dev = torch.from_numpy(frames[:n]).cuda()
    mbuf, mview = guarded(n * 8192, 0, 8192, GUARD)
    abuf, aview = guarded(n * 8192, 0, 8192, GUARD)
    native.frames_to_memory_maps(mode, O.PALETTE_RGB[5], dev, dither, out=(mview, aview))
    torch.cuda.synchronize()
    got = mbuf.cpu().numpy().reshape(n + 1, 32, 256)
    for i in range(n):
        assert (got[i] == em[i]).all(), (mode, dither, n, i, int((got[i] != em[i]).sum()))
    assert (got[n] == GUARD).all()
    got = abuf.cpu().numpy().reshape(n + 1, 32, 256)
    if mode == M.DHGR:
        for i in range(n):
            assert (got[i] == ea[i]).all(), (mode, dither, n, i, "aux", int((got[i] != ea[i]).sum()))
        assert (got[n] == GUARD).all()
    else:
        assert (got == GUARD).all()          # HGR has no aux bank: none of it is touched


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dither", [32, M.DITHER_DIFFUSION])
def test_source_offsets(native, O, mode, dither):
    """The batch as a view 0, 4, 8, 12, 20, 36, 60 bytes into a larger allocation: the same bytes out, the oracle's."""
    import torch
    n = 7
    frames, em, ea = _batch(O, mode, dither)
    flat = torch.from_numpy(frames[:n].reshape(-1))
    buf = torch.full((n * FRAME_BYTES + 64,), GUARD, dtype=torch.uint8, device="cuda")
    first = None
    for o in (0, 4, 8, 12, 20, 36, 60):
        buf.fill_(GUARD)
        buf[o:o + n * FRAME_BYTES] = flat.cuda()
        src = buf[o:o + n * FRAME_BYTES].view(n, 192, 280, 3)
        assert src.data_ptr() == buf.data_ptr() + o and src.is_contiguous()
        main, aux = native.frames_to_memory_maps(mode, O.PALETTE_RGB[5], src, dither)
        main = main.cpu().numpy()
        aux = aux.cpu().numpy() if aux is not None else None
        for i in range(n):
            assert (main[i] == em[i]).all(), (mode, dither, o, i, int((main[i] != em[i]).sum()))
            if mode == M.DHGR:
                assert (aux[i] == ea[i]).all(), (mode, dither, o, i, "aux", int((aux[i] != ea[i]).sum()))
        if first is None:
            first = (main, aux)
        else:
            assert (main == first[0]).all() and (aux is None or (aux == first[1]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dither", [32, M.DITHER_DIFFUSION])
def test_output_offsets(native, O, mode, dither):
    """out= views 8 and 24 bytes into larger buffers (main and aux at different ones): the oracle's bytes inside, the fill
    around them."""
    import torch
    n = 7
    frames, em, ea = _batch(O, mode, dither)
    dev = torch.from_numpy(frames[:n]).cuda()
    for om, oa in ((8, 24), (24, 8)):
        mbuf, mview = guarded(n * 8192, om, 40, GUARD)
        abuf, aview = guarded(n * 8192, oa, 40, GUARD)
        assert mview.data_ptr() % 16 == 8 and aview.data_ptr() % 16 == 8
        native.frames_to_memory_maps(mode, O.PALETTE_RGB[5], dev, dither, out=(mview.view(n, 32, 256), aview.view(n, 32, 256)))
        torch.cuda.synchronize()
        got = mview.cpu().numpy().reshape(n, 32, 256)
        for i in range(n):
            assert (got[i] == em[i]).all(), (mode, dither, om, i, int((got[i] != em[i]).sum()))
        assert guards_kept(mbuf, om, n * 8192, GUARD)
        if mode == M.DHGR:
            got = aview.cpu().numpy().reshape(n, 32, 256)
            for i in range(n):
                assert (got[i] == ea[i]).all(), (mode, dither, oa, i, "aux", int((got[i] != ea[i]).sum()))
            assert guards_kept(abuf, oa, n * 8192, GUARD)
        else:
            assert (abuf.cpu().numpy() == GUARD).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dither", [32, M.DITHER_DIFFUSION])
def test_misaligned_arguments_are_refused_and_nothing_is_written(native, O, mode, dither):
    """The contract: d_rgb 4-byte aligned, d_main / d_aux 8-byte aligned.  Anything less is IIV_ERR_INVALID before a kernel
    is launched."""
    import torch
    n = 2
    frames, _, _ = _batch(O, mode, dither)
    pal = O.PALETTE_RGB[5]
    src_buf = torch.zeros((n * FRAME_BYTES + 16,), dtype=torch.uint8, device="cuda")
    src_buf[:n * FRAME_BYTES] = torch.from_numpy(frames[:n].reshape(-1)).cuda()
    mbuf, mview = guarded(n * 8192, 8, 8, GUARD)
    abuf, aview = guarded(n * 8192, 8, 8, GUARD)

    def untouched():
        torch.cuda.synchronize()
        return (mbuf.cpu().numpy() == GUARD).all() and (abuf.cpu().numpy() == GUARD).all()

    for o in (1, 2):
        src = src_buf[o:o + n * FRAME_BYTES].view(n, 192, 280, 3)
        with pytest.raises(native.IIVError):
            native.frames_to_memory_maps(mode, pal, src, dither, out=(mview, aview))
        assert untouched(), ("source offset", o)
    src = src_buf[:n * FRAME_BYTES].view(n, 192, 280, 3)
    main4_buf, main4 = guarded(n * 8192, 4, 4, GUARD)
    with pytest.raises(native.IIVError):
        native.frames_to_memory_maps(mode, pal, src, dither, out=(main4, aview))
    torch.cuda.synchronize()
    assert (main4_buf.cpu().numpy() == GUARD).all() and untouched(), "main offset 4"
    if mode == M.DHGR:
        aux4_buf, aux4 = guarded(n * 8192, 4, 4, GUARD)
        with pytest.raises(native.IIVError):
            native.frames_to_memory_maps(mode, pal, src, dither, out=(mview, aux4))
        torch.cuda.synchronize()
        assert (aux4_buf.cpu().numpy() == GUARD).all() and untouched(), "aux offset 4"
    # and the aligned call on the same tensors goes through
    native.frames_to_memory_maps(mode, pal, src, dither, out=(mview, aview))
    torch.cuda.synchronize()
    assert not untouched()
