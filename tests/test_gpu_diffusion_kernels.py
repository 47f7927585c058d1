"""GPU: csrc/iiv_diffuse.hip (iiv_frames_to_memory_maps_diffused) byte for byte -- all (n, 32, 256) bytes of both banks --
against tests/diffusion_model.py, which tests/test_diffusion_model.py holds to the old contract and the oracle on the CPU.
  kernels        every named kernel and two made-up ones (see diffusion_model.MADE_UP: twelve distinct weights cannot sum
                 below 64, so two kernels of ten distinct values tell every pair of positions apart between them), both modes,
                 four frames of ingest_model.frame_set under a real palette and under a tie palette
  cross-check    Floyd-Steinberg's weights through the new entry point = the old entry point's bytes (two kernels)
  frame counts   1..7 and 13 for jarvis: one below, at and one above a wave's (three) and a workgroup's (six) share of frames,
                 guard bytes in front of and behind both banks
  offsets        the source at its least alignment (4 bytes), the outputs at theirs (8 bytes)
  refusals       every invalid argument of the contract is an IIVError and writes nothing
  upwards        ArrayFrameGrabber(dither=<name>) and tools/transcode_clip.py --dither <name>"""
import os
import subprocess
import sys

import numpy as np
import pytest

from device_guards import guarded, guards_kept
import diffusion_model as D
import ingest_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [M.DHGR, M.HGR]
FRAME_BYTES = 192 * 280 * 3
GUARD = 0xEE
KINDS = (0, 3, 4, 5)            # of ingest_model.FRAME_KINDS: noise, gradient, own colours, near colours
TIE_PALETTE = "hgr_ties_bw"     # blue == violet, orange == green, white == black: ties in DHGR's sixteen and in HGR's fours


def _kernel_of(name):
    return D.MADE_UP[int(name[-1])] if name.startswith("made-up") else D.KERNELS[name]


_cache = {}


def _sweep(O):
    """(palettes (8, 16, 3), frames (8, 192, 280, 3)): the four frames under the NTSC palette, then under the tie palette"""
    if "sweep" not in _cache:
        pals, frames = [], []
        for name in ("ntsc", TIE_PALETTE):
            p = M.palette(O, name)
            pals.append(np.broadcast_to(p, (len(KINDS), 16, 3)))
            frames.append(M.frames_of(O, name)[list(KINDS)])
        _cache["sweep"] = (np.concatenate(pals), np.concatenate(frames))
    return _cache["sweep"]


def _different_frames():
    """thirteen frames, no two alike: picture-like content and noise by turns"""
    if "different" not in _cache:
        rng = np.random.default_rng(78)
        y, x = np.mgrid[0:192, 0:280]
        out = np.empty((13, 192, 280, 3), np.uint8)
        for i in range(13):
            if i % 2:
                out[i] = rng.integers(0, 256, (192, 280, 3))
            else:
                out[i] = np.stack([(x + 23 * i) * 255 // 556, (y * (i + 3)) % 256, (x * 5 + y * 3 + 29 * i) % 256], axis=-1)
        _cache["different"] = out
    return _cache["different"]


def _jarvis_batch(O, mode):
    """(frames, expected main, expected aux) of the thirteen frames under the NTSC palette with jarvis: once per mode"""
    if ("jarvis", mode) not in _cache:
        w, d = D.KERNELS["jarvis"]
        _cache["jarvis", mode] = D.frames_to_memory_maps(mode, O.PALETTE_RGB[5], _different_frames(), w, d)
    return (_different_frames(),) + _cache["jarvis", mode]


def _assert_banks(got_main, got_aux, em, ea, mode, what):
    got_main = got_main.cpu().numpy().reshape(em.shape)
    for i in range(len(em)):
        assert (got_main[i] == em[i]).all(), what + (i, "main", int((got_main[i] != em[i]).sum()))
    if mode == M.DHGR:
        got_aux = got_aux.cpu().numpy().reshape(ea.shape)
        for i in range(len(ea)):
            assert (got_aux[i] == ea[i]).all(), what + (i, "aux", int((got_aux[i] != ea[i]).sum()))
    else:
        assert got_aux is None and ea is None


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(D.KERNELS) + ["made-up 0", "made-up 1"])
def test_kernels_equal_the_model(native, O, name, mode):
    import torch
    pals, frames = _sweep(O)
    w, d = _kernel_of(name)
    em, ea = D.frames_to_memory_maps(mode, pals, frames, w, d)
    half = len(KINDS)
    for p in range(2):       # one call per palette
        dev = torch.from_numpy(frames[p * half:(p + 1) * half]).cuda()
        main, aux = native.frames_to_memory_maps_diffused(mode, pals[p * half], dev, w, d)
        _assert_banks(main, aux, em[p * half:(p + 1) * half], ea[p * half:(p + 1) * half] if ea is not None else None, mode,
                      (name, mode, ("ntsc", TIE_PALETTE)[p]))


@pytest.mark.parametrize("mode", MODES)
def test_floyd_steinberg_weights_equal_the_old_entry_point(native, O, mode):
    """two kernels, one contract: the new one with {7 | 3 5 1} / 16 against ingest_diffusion_kernel"""
    import torch
    w, d = D.KERNELS["floyd-steinberg"]
    pals, frames = _sweep(O)
    half = len(KINDS)
    for pal, fr in ((pals[0], frames[:half]), (pals[half], frames[half:]), (O.PALETTE_RGB[0], _different_frames())):
        dev = torch.from_numpy(np.ascontiguousarray(fr)).cuda()
        new_main, new_aux = native.frames_to_memory_maps_diffused(mode, pal, dev, w, d)
        old_main, old_aux = native.frames_to_memory_maps(mode, pal, dev, native.DITHER_DIFFUSION)
        assert torch.equal(new_main, old_main), (mode, int((new_main != old_main).sum()))
        assert (new_aux is None and old_aux is None) if mode == M.HGR else torch.equal(new_aux, old_aux)
        assert new_main.any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 6, 7, 13))
def test_frame_counts_and_guards(native, O, mode, n):
    """n different frames into buffers with a frame's worth of guard bytes in front and behind: frames 0 .. n - 1 are the
    model's (holes zero), the guards keep their fill"""
    import torch
    frames, em, ea = _jarvis_batch(O, mode)
    w, d = D.KERNELS["jarvis"]
    dev = torch.from_numpy(frames[:n]).cuda()
    mbuf, mview = guarded(n * 8192, 8192, 8192, GUARD)
    abuf, aview = guarded(n * 8192, 8192, 8192, GUARD)
    native.frames_to_memory_maps_diffused(mode, O.PALETTE_RGB[5], dev, w, d, out=(mview, aview))
    torch.cuda.synchronize()
    _assert_banks(mview, aview if mode == M.DHGR else None, em[:n], ea[:n] if ea is not None else None, mode, ("jarvis", mode, n))
    assert guards_kept(mbuf, 8192, n * 8192, GUARD)
    if mode == M.DHGR:
        assert guards_kept(abuf, 8192, n * 8192, GUARD)
    else:
        assert (abuf.cpu().numpy() == GUARD).all()          # HGR has no aux bank: none of it is touched


@pytest.mark.parametrize("mode", MODES)
def test_least_alignments(native, O, mode):
    """the source 4 bytes into its allocation, main and aux 8 bytes into theirs: the model's bytes inside, the fill around"""
    import torch
    n = 7
    frames, em, ea = _jarvis_batch(O, mode)
    w, d = D.KERNELS["jarvis"]
    sbuf = torch.full((n * FRAME_BYTES + 64,), GUARD, dtype=torch.uint8, device="cuda")
    sbuf[4:4 + n * FRAME_BYTES] = torch.from_numpy(frames[:n].reshape(-1)).cuda()
    src = sbuf[4:4 + n * FRAME_BYTES].view(n, 192, 280, 3)
    mbuf, mview = guarded(n * 8192, 8, 40, GUARD)
    abuf, aview = guarded(n * 8192, 8, 40, GUARD)
    assert src.data_ptr() % 8 == 4 and mview.data_ptr() % 16 == 8 and aview.data_ptr() % 16 == 8
    native.frames_to_memory_maps_diffused(mode, O.PALETTE_RGB[5], src, w, d, out=(mview, aview))
    torch.cuda.synchronize()
    _assert_banks(mview, aview if mode == M.DHGR else None, em[:n], ea[:n] if ea is not None else None, mode, ("offsets", mode))
    assert guards_kept(mbuf, 8, n * 8192, GUARD)
    assert guards_kept(abuf, 8, n * 8192, GUARD) if mode == M.DHGR else bool((abuf.cpu().numpy() == GUARD).all())


@pytest.mark.parametrize("mode", MODES)
def test_invalid_arguments_are_refused_and_nothing_is_written(native, O, mode):
    import ctypes
    import torch
    n = 2
    frames = _different_frames()
    pal = np.ascontiguousarray(O.PALETTE_RGB[5], dtype=np.uint8).reshape(48)
    jarvis, jd = D.KERNELS["jarvis"]
    src_buf = torch.zeros((n * FRAME_BYTES + 16,), dtype=torch.uint8, device="cuda")
    src_buf[:n * FRAME_BYTES] = torch.from_numpy(frames[:n].reshape(-1)).cuda()
    src = src_buf[:n * FRAME_BYTES].view(n, 192, 280, 3)
    mbuf, mview = guarded(n * 8192, 8, 8, GUARD)
    abuf, aview = guarded(n * 8192, 8, 8, GUARD)

    def untouched():
        torch.cuda.synchronize()
        return bool((mbuf.cpu().numpy() == GUARD).all() and (abuf.cpu().numpy() == GUARD).all())

    def refused(what, rgb=src, weights=jarvis, divisor=jd, out=None):
        with pytest.raises(native.IIVError) as info:
            native.frames_to_memory_maps_diffused(mode, pal, rgb, weights, divisor, out=out or (mview, aview))
        assert info.value.code == native.ERR_INVALID, what
        assert untouched(), what

    # the divisor's range
    for divisor in (0, -1, 65, 1 << 20):
        refused(("divisor", divisor), weights=np.zeros(15, np.uint8), divisor=divisor)
    # the pixel itself and what lies left of it
    for j in range(3):
        w = D.KERNELS["floyd-steinberg"][0].reshape(15).copy()
        w[j] = 1
        w[3] = 6
        refused(("weights", j), weights=w, divisor=16)
    # a sum above the divisor (by one; and a sum that only fits a wider type)
    refused("sum 48 > 47", divisor=47)
    refused("sum 15 x 255", weights=np.full(15, 255, np.uint8) * (np.arange(15) > 2), divisor=64)
    # alignments, as for iiv_frames_to_memory_maps
    for o in (1, 2):
        refused(("source offset", o), rgb=src_buf[o:o + n * FRAME_BYTES].view(n, 192, 280, 3))
    main4_buf, main4 = guarded(n * 8192, 4, 4, GUARD)
    refused("main offset 4", out=(main4, aview))
    assert (main4_buf.cpu().numpy() == GUARD).all()
    if mode == M.DHGR:
        aux4_buf, aux4 = guarded(n * 8192, 4, 4, GUARD)
        refused("aux offset 4", out=(mview, aux4))
        assert (aux4_buf.cpu().numpy() == GUARD).all()
    # a bad mode: through the C ABI itself
    rc = native.lib().iiv_frames_to_memory_maps_diffused(2, native.hptr(pal), n, native.dptr(src), native.hptr(np.zeros(15, np.uint8)), 16,
                                                         native.dptr(mview), native.dptr(aview), native.stream_ptr())
    assert rc == native.ERR_INVALID and untouched()
    # and the legal call on the same tensors goes through: a sum equal to the divisor, and no weights at all
    native.frames_to_memory_maps_diffused(mode, pal, src, jarvis, jd, out=(mview, aview))
    assert not untouched()
    native.frames_to_memory_maps_diffused(mode, pal, src, np.zeros((3, 5), np.uint8), 1, out=(mview, aview))
    torch.cuda.synchronize()


def test_dhgr_without_weights_is_the_conversion_without_dither(native, O):
    import torch
    dev = torch.from_numpy(_different_frames()[:4]).cuda()
    main, aux = native.frames_to_memory_maps_diffused(M.DHGR, O.PALETTE_RGB[5], dev, np.zeros((3, 5), np.uint8), 64)
    em, ea = native.frames_to_memory_maps(M.DHGR, O.PALETTE_RGB[5], dev, 0)
    assert torch.equal(main, em) and torch.equal(aux, ea)


@pytest.mark.parametrize("mode", MODES)
def test_frame_grabber_by_name_and_by_weights(native, O, mode):
    import torch
    import frame_grabber
    import palette as palette_mod
    from palette import Palette
    from video_mode import VideoMode
    frames = _different_frames()[:4]
    vm = VideoMode.DHGR if mode == M.DHGR else VideoMode.HGR
    w, d = D.KERNELS["atkinson"]
    pal = palette_mod.PALETTES[Palette.NTSC].rgb_array()
    em, ea = native.frames_to_memory_maps_diffused(mode, pal, torch.from_numpy(frames).cuda(), w, d)
    for dither in ("atkinson", (w, d), (w.tolist(), d)):
        main, aux = frame_grabber.ArrayFrameGrabber(frames, vm, Palette.NTSC, dither=dither).memory_maps()
        assert torch.equal(main, em) and (aux is None if mode == M.HGR else torch.equal(aux, ea))
    # and not the old kernel's bytes under another name
    old, _ = frame_grabber.ArrayFrameGrabber(frames, vm, Palette.NTSC, dither="diffusion").memory_maps()
    assert not torch.equal(old, em)
    with pytest.raises(ValueError):
        frame_grabber.ArrayFrameGrabber(frames, vm, Palette.NTSC, dither="atkinsen")
    mono = np.zeros((1,) + native.MONO_SIZE[mode] + (3,), np.uint8)
    with pytest.raises(ValueError):
        frame_grabber.ArrayFrameGrabber(mono, vm, Palette.MONO, dither="atkinson")
    frame_grabber.ArrayFrameGrabber(mono, vm, Palette.MONO, dither="diffusion")


@pytest.mark.parametrize("mode_name", ["DHGR", "HGR"])
def test_transcode_clip_with_a_named_kernel_equals_the_model_chain(tmp_path, O, oracle_tables, mode_name):
    """tools/transcode_clip.py --synthetic 6 --dither atkinson: the file's bytes are those of the same chain through the model
    of the conversion and the oracle's encoder and emitter (tests/test_gpu_transcode_tool.py does this for the default)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import stream_batch
    import transcode_clip
    n = 6
    out = tmp_path / "clip.a2m"
    args = [sys.executable, os.path.join(ROOT, "tools", "transcode_clip.py"), "--synthetic", str(n), "--out", str(out),
            "--mode", mode_name, "--seed", "7", "--tick", "20", "--dither", "atkinson"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "dither atkinson" in r.stdout
    got = np.frombuffer(out.read_bytes(), np.uint8)

    mode = 1 if mode_name == "DHGR" else 0
    w, d = D.KERNELS["atkinson"]
    mm, ma = D.frames_to_memory_maps(mode, O.PALETTE_RGB[5], transcode_clip.test_card(n), w, d)
    v = O.Video(mode, oracle_tables.get(mode, 5), seed_py=7, seed_np=7)
    ops = []
    for (fr, ia, restart, k) in stream_batch.MovieClock(mode == 1).segments(n):
        if restart:
            v.encode_frame(mm[fr], ma[fr] if mode == 1 else None, ia)
        ops.append(v.next(k))
    ops = np.concatenate(ops)
    tick_addr = (0x8000 + 16 * np.arange(1024)).astype(np.uint16)
    exp = O.emit_stream(mode, ops, np.full(len(ops), 20, np.uint8), tick_addr, 0xc000, 0xc100)
    assert len(got) == len(exp) and len(got) % 2048 == 0
    assert (got == exp).all()
