"""GPU: iiv_frames_to_memory_maps_direct (csrc/iiv_direct.hip) against tests/direct_model.py, the numpy restatement of
"f10: direct ingest" in include/iivision.h.  Every comparison is == on bytes and on uint64 costs.
  kernel = model     both modes x both source widths x NTSC, IIGS and a palette of duplicate colours (heavy ties) x dither 0, 32,
                     255; noise, the test card, all-black and all-white frames; 5 frames, the first 3, and each alone (192, 576
                     and 960 rows: partly filled workgroups of 64 and 32 rows)
  screen error       dither 0: d_cost is iiv_render_error's level 0 of the kernel's own maps, summed over the channels
  other converters   d_cost <= that sum for iiv_frames_to_memory_maps' maps (ordered and diffusion) of the same frames
  buffers            guarded outputs on both sides, d_cost == NULL, d_rgb 4 bytes off 16, maps 8 bytes off 16
  refusals           every invalid argument of the contract: IIV_ERR_INVALID, the function named, sentinel outputs untouched
  side stream        one call on a busy non-blocking stream (tests/stream_probe.py): decoy inputs, sentinel outputs, the palette
                     overwritten right after the call
  Python layer       ArrayFrameGrabber(dither="direct"); transcode_clip.py --dither direct --quality: the .a2m bytes of the same
                     chain through the model and the oracle's encoder"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import direct_model as D
import ingest_model
import render_error_model as E
import render_model as R
import stream_probe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [R.HGR, R.DHGR]
WIDTHS = [280, 560]
DITHERS = [0, 32, 255]
FILL = 0xC3


def _palette(name):
    import palette
    if name == "PAIRS":
        return ingest_model.PALETTES["pairs"]
    return np.asarray({"NTSC": palette.NTSCPalette, "IIGS": palette.IIGSPalette}[name].rgb_array(), dtype=np.uint8).reshape(16, 3)


def _card(n, width):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import transcode_clip
    return np.ascontiguousarray(transcode_clip.test_card(n, width))


def _frames(width, seed):
    """(5, 192, width, 3): noise, the test card, black, white, noise"""
    rng = np.random.default_rng(seed)
    out = np.empty((5, 192, width, 3), np.uint8)
    out[0], out[4] = rng.integers(0, 256, (2, 192, width, 3))
    out[1] = _card(1, width)[0]
    out[2], out[3] = 0, 255
    return out


def _convert(native, mode, pal, rgb, dither, cost=True):
    import torch
    got = native.frames_to_memory_maps_direct(mode, pal, torch.from_numpy(np.ascontiguousarray(rgb)).cuda(), dither, cost=cost)
    return [None if t is None else t.cpu().numpy() for t in got]


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert (got == want).all(), (what, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("pal_name", ["NTSC", "IIGS", "PAIRS"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_kernel_equals_model(native, mode, width, pal_name):
    pal, rgb = _palette(pal_name), _frames(width, 31 * width + mode)
    for dither in DITHERS:
        wmain, waux, wcost = D.frames_to_memory_maps_direct(mode, pal, rgb, dither)
        for pick in (slice(0, 5), slice(0, 3)) + tuple(slice(k, k + 1) for k in range(5)):
            main, aux, cost = _convert(native, mode, pal, rgb[pick], dither)
            what = (dither, pick.start, pick.stop)
            _same(main, wmain[pick], what + ("main",))
            if mode == R.DHGR:
                _same(aux, waux[pick], what + ("aux",))
            else:
                assert aux is None
            assert cost.dtype == np.uint64
            _same(cost, wcost[pick], what + ("cost",))


def _level0(native, mode, pal, main, aux, rgb):
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return native.render_error(mode, pal, t(main), t(aux), t(rgb)).cpu().numpy()[:, 0, :].sum(axis=1)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_cost_is_render_error_level_0_and_never_above_the_other_converters(native, mode, width):
    import torch
    pal, rgb = _palette("NTSC"), _frames(width, 77 + width + mode)
    main, aux, cost = _convert(native, mode, pal, rgb, 0)
    print("d_cost", cost.tolist())
    own = _level0(native, mode, pal, main, aux, rgb)
    assert (cost == own).all(), (cost.tolist(), own.tolist())
    if width == 280:
        d = torch.from_numpy(rgb).cuda()
        for dither in (0, 32, native.DITHER_DIFFUSION):
            om, oa = native.frames_to_memory_maps(mode, pal, d, dither)
            other = _level0(native, mode, pal, om.cpu().numpy(), None if oa is None else oa.cpu().numpy(), rgb)
            print("dither", dither, other.tolist())
            assert (cost <= other).all(), (dither, cost.tolist(), other.tolist())


def _guarded(torch, n_bytes, lead, trail):
    buf = torch.full((lead + n_bytes + trail,), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + n_bytes]


@pytest.mark.parametrize("mode", MODES)
def test_guards_least_alignments_and_no_cost(native, mode):
    """Outputs between guard bytes at the least alignment the contract allows (8 bytes off 16), the source 4 bytes off 16, and
    a call without d_cost: the maps are the model's, the guards untouched."""
    import torch
    n, width = 3, 280
    pal, rgb = _palette("IIGS"), _frames(width, 400 + mode)[[0, 1, 4]]
    wmain, waux, wcost = D.frames_to_memory_maps_direct(mode, pal, rgb, 32)
    hp = np.ascontiguousarray(pal).reshape(48)
    src_buf = torch.zeros(rgb.size + 32, dtype=torch.uint8, device="cuda")
    assert src_buf.data_ptr() % 16 == 0
    src = src_buf[4:4 + rgb.size]
    src.copy_(torch.from_numpy(rgb.reshape(-1)).cuda())
    mbuf, m = _guarded(torch, n * 8192, 24, 40)
    abuf, a = _guarded(torch, n * 8192, 8, 8)
    cbuf, c = _guarded(torch, n * 8, 8, 8)
    assert m.data_ptr() % 16 == 8 and a.data_ptr() % 16 == 8 and c.data_ptr() % 16 == 8 and src.data_ptr() % 16 == 4
    L, st = native.lib(), native.stream_ptr()
    for with_cost in (True, False):
        for b in (m, a, c):
            b.fill_(FILL)
        rc = L.iiv_frames_to_memory_maps_direct(mode, native.hptr(hp), n, native.dptr(src), width, 32, native.dptr(m),
                                                native.dptr(a) if mode == R.DHGR else None, native.dptr(c) if with_cost else None, st)
        assert rc == 0, L.iiv_last_error()
        torch.cuda.synchronize()
        _same(m.cpu().numpy().reshape(n, 32, 256), wmain, "main")
        if mode == R.DHGR:
            _same(a.cpu().numpy().reshape(n, 32, 256), waux, "aux")
        else:
            assert (a.cpu().numpy() == FILL).all()
        if with_cost:
            _same(c.cpu().numpy().view(np.uint64), wcost, "cost")
        else:
            assert (c.cpu().numpy() == FILL).all()
        for buf, lead, size in ((mbuf, 24, n * 8192), (abuf, 8, n * 8192), (cbuf, 8, n * 8)):
            h = buf.cpu().numpy()
            assert (h[:lead] == FILL).all() and (h[lead + size:] == FILL).all()


def test_refusals_write_nothing(native):
    import torch
    n = 2
    rgb = torch.zeros((n, 192, 560, 3), dtype=torch.uint8, device="cuda")
    main = torch.full((n + 1, 32, 256), FILL, dtype=torch.uint8, device="cuda")
    aux = torch.full((n + 1, 32, 256), FILL, dtype=torch.uint8, device="cuda")
    cost = torch.full((8 * (n + 1),), FILL, dtype=torch.uint8, device="cuda")
    hp = np.ascontiguousarray(_palette("NTSC")).reshape(48)
    L, st = native.lib(), native.stream_ptr()
    r, m, a, c = rgb.data_ptr(), main.data_ptr(), aux.data_ptr(), cost.data_ptr()

    def call(mode, count, pr, width, dither, pm, pa, pc, pal=hp):
        return L.iiv_frames_to_memory_maps_direct(mode, None if pal is None else native.hptr(pal), count, C.c_void_p(pr), width, dither,
                                                  C.c_void_p(pm), C.c_void_p(pa), C.c_void_p(pc), st)

    refused = {"mode 2": (2, n, r, 560, 0, m, a, c), "mode -1": (-1, n, r, 560, 0, m, a, c), "n < 0": (R.DHGR, -1, r, 560, 0, m, a, c),
               "no source": (R.HGR, n, 0, 560, 0, m, a, c), "no main": (R.HGR, n, r, 560, 0, 0, a, c),
               "DHGR without aux": (R.DHGR, n, r, 560, 0, m, 0, c), "width 0": (R.DHGR, n, r, 0, 0, m, a, c),
               "width 140": (R.HGR, n, r, 140, 0, m, a, c), "width 281": (R.DHGR, n, r, 281, 0, m, a, c),
               "width 1120": (R.HGR, n, r, 1120, 0, m, a, c), "dither -1": (R.DHGR, n, r, 560, -1, m, a, c),
               "dither 256 (diffusion)": (R.DHGR, n, r, 560, native.DITHER_DIFFUSION, m, a, c), "dither 257": (R.HGR, n, r, 560, 257, m, a, c),
               "source off by 2": (R.DHGR, 1, r + 2, 280, 0, m, a, c), "source off by 1": (R.HGR, 1, r + 1, 560, 0, m, a, c),
               "main off by 4": (R.HGR, 1, r, 560, 0, m + 4, a, c), "aux off by 4": (R.DHGR, 1, r, 560, 0, m, a + 4, c),
               "cost off by 4": (R.DHGR, 1, r, 560, 0, m, a, c + 4), "cost off by 1": (R.HGR, 1, r, 280, 0, m, a, c + 1)}
    for what, args in refused.items():
        assert call(*args) == native.ERR_INVALID, what
        assert b"iiv_frames_to_memory_maps_direct" in L.iiv_last_error(), what
    assert call(R.HGR, n, r, 560, 0, m, a, c, pal=None) == native.ERR_INVALID
    assert b"iiv_frames_to_memory_maps_direct" in L.iiv_last_error()
    assert call(R.DHGR, 0, r, 560, 0, m, a, c) == 0                  # n == 0 succeeds and writes nothing
    torch.cuda.synchronize()
    for t in (main, aux, cost):
        assert (t.cpu().numpy() == FILL).all()
    with pytest.raises(ValueError):
        native.frames_to_memory_maps_direct(R.DHGR, hp, rgb[:, :, :140])
    assert call(R.HGR, 1, r, 560, 0, m, a + 4, 0) == 0               # HGR does not look at d_aux, misaligned or not
    torch.cuda.synchronize()
    assert (aux.cpu().numpy() == FILL).all()


@pytest.mark.parametrize("mode", MODES)
def test_one_call_on_a_busy_side_stream(native, mode):
    n, width, dither = 2, 280, 32
    pal, other_pal = _palette("NTSC"), _palette("IIGS")
    frames = _frames(width, 900 + mode)
    real, decoy = frames[[0, 1]], frames[[4, 3]]
    wmain, waux, wcost = D.frames_to_memory_maps_direct(mode, pal, real, dither)
    native.frames_to_memory_maps_direct(mode, pal, native._torch().from_numpy(decoy).cuda(), dither, cost=True)   # warm-up
    p = stream_probe.Probe()
    src = p.input(real, decoy)
    main, aux, cost = p.output((n, 32, 256)), p.output((n, 32, 256)), p.output((n,), native._torch().uint64)
    hp = p.host(np.ascontiguousarray(pal).reshape(48), np.ascontiguousarray(other_pal).reshape(48))
    L = native.lib()
    rc = p.run(lambda st: L.iiv_frames_to_memory_maps_direct(mode, native.hptr(hp), n, native.dptr(src), width, dither, native.dptr(main),
                                                             native.dptr(aux), native.dptr(cost), st))
    assert rc == 0, L.iiv_last_error()
    _same(main.cpu().numpy(), wmain, "main")
    if mode == R.DHGR:
        _same(aux.cpu().numpy(), waux, "aux")
    else:
        assert (aux.cpu().numpy() == stream_probe.SENTINEL_B).all()
    _same(cost.cpu().numpy(), wcost, "cost")


def test_array_frame_grabber_direct(native):
    import frame_grabber
    import palette
    import video_mode
    rgb = _frames(280, 5)[[0, 1]]
    pal = _palette("NTSC")
    for mode, vm in ((R.HGR, video_mode.VideoMode.HGR), (R.DHGR, video_mode.VideoMode.DHGR)):
        for amplitude in (0, 32):
            grab = frame_grabber.ArrayFrameGrabber(rgb, vm, palette.Palette.NTSC, dither="direct", amplitude=amplitude)
            main, aux = grab.memory_maps()
            wmain, waux, _ = D.frames_to_memory_maps_direct(mode, pal, rgb, amplitude)
            _same(main.cpu().numpy(), wmain, (mode, amplitude))
            if mode == R.DHGR:
                _same(aux.cpu().numpy(), waux, (mode, amplitude))
    with pytest.raises(ValueError):
        frame_grabber.ArrayFrameGrabber(rgb, video_mode.VideoMode.DHGR, palette.Palette.NTSC, dither=32, amplitude=8)
    with pytest.raises(ValueError):
        frame_grabber.ArrayFrameGrabber(rgb, video_mode.VideoMode.DHGR, palette.Palette.NTSC, dither="diffusion", amplitude=8)
    with pytest.raises(ValueError):
        frame_grabber.ArrayFrameGrabber(np.zeros((1, 192, 560, 3), np.uint8), video_mode.VideoMode.DHGR, palette.Palette.MONO, dither="direct")
    with pytest.raises(ValueError):
        frame_grabber.ArrayFrameGrabber(rgb, video_mode.VideoMode.DHGR, palette.Palette.NTSC, dither="direct", amplitude=256)


@pytest.mark.parametrize("mode_name,amplitude", [("DHGR", 0), ("HGR", 32)])
def test_transcode_clip_direct_equals_the_model_and_oracle_chain(native, tmp_path, O, oracle_tables, mode_name, amplitude):
    """tools/transcode_clip.py --synthetic 3 --dither direct [--amplitude N] --quality: the .a2m bytes are those of the same
    chain through the model's maps and the oracle's encoder and emitter (as tests/test_gpu_transcode_tool.py does for the other
    dithers), and the quality file holds the model's sums for the tool's own previews."""
    import stream_batch
    n = 3
    out = tmp_path / "d.a2m"
    tool = [sys.executable, os.path.join(ROOT, "tools", "transcode_clip.py"), "--synthetic", str(n), "--seed", "7", "--tick", "20",
            "--mode", mode_name, "--dither", "direct", "--amplitude", str(amplitude), "--out", str(out),
            "--preview", str(tmp_path / "d.npy"), "--quality", str(tmp_path / "q.json")]
    r = subprocess.run(tool, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer(out.read_bytes(), np.uint8)
    card = _card(n, 280)
    mode = 1 if mode_name == "DHGR" else 0
    wmain, waux, _ = D.frames_to_memory_maps_direct(mode, O.PALETTE_RGB[5], card, amplitude)
    v = O.Video(mode, oracle_tables.get(mode, 5), seed_py=7, seed_np=7)
    ops = []
    for (fr, ia, restart, k) in stream_batch.MovieClock(mode == 1).segments(n):
        if restart:
            v.encode_frame(wmain[fr], waux[fr] if mode == 1 else None, ia)
        ops.append(v.next(k))
    ops = np.concatenate(ops)
    tick_addr = (0x8000 + 16 * np.arange(1024)).astype(np.uint16)
    exp = O.emit_stream(mode, ops, np.full(len(ops), 20, np.uint8), tick_addr, 0xc000, 0xc100)
    assert len(got) == len(exp) and len(got) % 2048 == 0
    assert (got == exp).all()
    with open(tmp_path / "q.json") as f:
        q = json.load(f)
    want = E.error_sums_of_screens(np.load(tmp_path / "d.npy"), card)
    assert [fr["sums"] for fr in q["frames"]] == want.tolist()
