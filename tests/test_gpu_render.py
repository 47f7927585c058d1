"""GPU: iiv_render_rgb / iiv_encoder_render (csrc/iiv_render.hip) -- screen memory to 560 x 192 RGB -- against
tests/render_model.py, the numpy restatement of the contract in include/iivision.h that tests/test_render_model.py holds to
the reference-recorded colour strings.  Byte for byte, in both modes:
  kernel = model   random screens (random bytes in the holes too) at 1, 3 and 5 frames -- 105, 315 and 525 wave runs, none a
                   multiple of the four runs of a workgroup --, constant and alternating screens, four palettes
  bounds           guard bytes around an output at its least alignment, inputs at theirs
  refusals         every invalid argument of the contract is IIV_ERR_INVALID and writes nothing; n = 0 is a success
  round trip       a card of the sixteen colours through iiv_frames_to_memory_maps and back
  encoder          iiv_encoder_render = iiv_render_rgb of the maps read back, and leaves the encoder as it was
  Python layer     screen.render_rgb, StreamBatch.screens_rgb, Video.screen_rgb, transcode_clip.py --preview"""
import contextlib
import ctypes as C
import io
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from device_guards import guarded
import encode_harness as H
import render_model as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [R.HGR, R.DHGR]
GUARD = 0xA5
FRAME = 192 * 560 * 3

# 48 distinct bytes: a swapped channel or colour index changes a pixel
DISTINCT = ((np.arange(48) * 37 + 11) % 256).astype(np.uint8).reshape(16, 3)
assert len(set(DISTINCT.reshape(-1).tolist())) == 48


def _palettes():
    import palette
    return {"distinct": DISTINCT, "NTSC": palette.NTSCPalette.rgb_array(), "IIGS": palette.IIGSPalette.rgb_array(),
            "MONO": palette.MonoPalette.rgb_array()}


def _random_screens(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 32, 256), dtype=np.uint8), rng.integers(0, 256, (n, 32, 256), dtype=np.uint8)


def _render(native, mode, pal, main, aux):
    import torch
    dm = torch.from_numpy(main).cuda()
    da = torch.from_numpy(aux).cuda() if mode == R.DHGR else None
    return native.render_rgb(mode, pal, dm, da).cpu().numpy()


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    return "first of %d differing bytes at (frame, y, x, channel) = %s: %d, model %d" % (
        len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]) if len(bad) else ""


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("mode", MODES)
def test_kernel_equals_model_on_random_screens(native, mode, n):
    main, aux = _random_screens(n, 100 * mode + n)
    got = _render(native, mode, DISTINCT, main, aux)
    want = R.render_rgb(mode, main, aux, DISTINCT)
    assert got.shape == (n, 192, 560, 3) and got.dtype == np.uint8
    assert (got == want).all(), _first_difference(got, want)


@pytest.mark.parametrize("pal_name", ["distinct", "NTSC", "IIGS", "MONO"])
@pytest.mark.parametrize("mode", MODES)
def test_constant_and_alternating_screens_in_every_palette(native, mode, pal_name):
    pal = _palettes()[pal_name]
    alt = np.where(np.arange(8192) & 1, 0x7f, 0x80).astype(np.uint8).reshape(32, 256)
    rnd = _random_screens(1, 9)
    main = np.stack([np.full((32, 256), v, np.uint8) for v in (0x00, 0x7f, 0xff)] + [alt, rnd[0][0]])
    aux = np.stack([np.full((32, 256), v, np.uint8) for v in (0x00, 0x7f, 0xff)] + [alt, rnd[1][0]])
    got = _render(native, mode, pal, main, aux)
    want = R.render_rgb(mode, main, aux, pal)
    assert (got == want).all(), _first_difference(got, want)
    assert (got[0] == pal[0]).all()                       # a dark screen is colour value 0 everywhere
    assert (got[1, :, 3:] == pal[15]).all()               # every dot lit: white from the fourth dot on


@pytest.mark.parametrize("mode", MODES)
def test_guards_and_least_alignments(native, mode):
    """The output sliced from a larger allocation at 16 bytes and no more, the inputs at 8: the 64 bytes in front of and behind
    the output keep their fill."""
    import torch
    n = 2
    main, aux = _random_screens(n, 40 + mode)
    mbuf, mview = guarded(n * 8192, 8, 8, GUARD)
    abuf, aview = guarded(n * 8192, 8, 8, GUARD)
    mview.copy_(torch.from_numpy(main).reshape(-1))
    aview.copy_(torch.from_numpy(aux).reshape(-1))
    obuf, oview = guarded(n * FRAME, 64 + 16, 64, GUARD)
    assert oview.data_ptr() % 32 == 16 and mview.data_ptr() % 16 == 8 and aview.data_ptr() % 16 == 8
    got = native.render_rgb(mode, DISTINCT, mview, aview if mode == R.DHGR else None, out=oview).cpu().numpy()
    want = R.render_rgb(mode, main, aux, DISTINCT)
    assert (got == want).all(), _first_difference(got, want)
    whole = obuf.cpu().numpy()
    assert (whole[:80] == GUARD).all() and (whole[80 + n * FRAME:] == GUARD).all()
    assert (mbuf.cpu().numpy()[8:-8] == main.reshape(-1)).all()      # (the inputs are only read)


def test_refusals_write_nothing(native):
    import torch
    L = native.lib()
    n = 2
    main, aux = _random_screens(n, 77)
    dm, da = torch.from_numpy(main).cuda(), torch.from_numpy(aux).cuda()
    pal = np.ascontiguousarray(DISTINCT).reshape(48)
    obuf, oview = guarded(n * FRAME, 64, 64, GUARD)
    st = native.stream_ptr()

    def call(mode, count, pm, pa, po):
        return L.iiv_render_rgb(mode, native.hptr(pal), count, C.c_void_p(pm), C.c_void_p(pa), C.c_void_p(po), st)

    m, a, o = dm.data_ptr(), da.data_ptr(), oview.data_ptr()
    refused = {"DHGR without aux": (R.DHGR, n, m, 0, o), "output off by 8": (R.DHGR, 1, m, a, o + 8),
               "output off by 1": (R.HGR, 1, m, a, o + 1), "main off by 4": (R.HGR, 1, m + 4, a, o),
               "aux off by 4": (R.DHGR, 1, m, a + 4, o), "mode 2": (2, n, m, a, o), "mode -1": (-1, n, m, a, o),
               "n < 0": (R.DHGR, -1, m, a, o), "no main": (R.HGR, n, 0, a, o), "no output": (R.HGR, n, m, a, 0)}
    for what, args in refused.items():
        assert call(*args) == native.ERR_INVALID, what
        assert b"iiv_render_rgb" in L.iiv_last_error(), what
    assert L.iiv_render_rgb(R.HGR, None, n, C.c_void_p(m), C.c_void_p(a), C.c_void_p(o), st) == native.ERR_INVALID   # no palette
    assert call(R.DHGR, 0, m, a, o) == 0 and call(R.HGR, 0, m, 0, o) == 0                 # n = 0: a success ...
    torch.cuda.synchronize()
    assert (obuf.cpu().numpy() == GUARD).all()                                            # ... and nothing was written by any of them
    # HGR needs no aux (an aux bank at a bad alignment is not looked at either)
    assert call(R.HGR, n, m, 0, o) == 0
    got = oview.cpu().numpy().reshape(n, 192, 560, 3)
    want = R.render_rgb(R.HGR, main, None, DISTINCT)
    assert (got == want).all(), _first_difference(got, want)
    assert call(R.HGR, n, m, a + 4, o) == 0
    assert (oview.cpu().numpy().reshape(n, 192, 560, 3) == want).all()


@pytest.mark.parametrize("pal_name", ["NTSC", "IIGS"])
def test_round_trip_of_a_colour_card(native, pal_name):
    """Sixteen vertical bars, sixteen source pixels (32 dots) wide, in the palette's own colours, through
    iiv_frames_to_memory_maps without dither and back: an aligned repeating quad P shows colour value P, so every dot at
    least four dots right of a bar's left edge is the bar's colour."""
    import torch
    pal = _palettes()[pal_name]
    card = np.zeros((1, 192, 280, 3), np.uint8)
    for b in range(16):
        card[:, :, 16 * b:16 * b + 16] = pal[b]
    card[:, :, 256:] = pal[0]
    main, aux = native.frames_to_memory_maps(R.DHGR, pal, torch.from_numpy(card).cuda(), 0)
    got = native.render_rgb(R.DHGR, pal, main, aux).cpu().numpy()[0]
    for b in range(16):
        assert (got[:, 32 * b + 4:32 * b + 32] == pal[b]).all(), "bar %d" % b
    assert (got[:, 512 + 4:] == pal[0]).all()


@pytest.mark.parametrize("mode", MODES)
def test_encoder_render(native, device_tables, mode):
    """Two streams, three frames of forty opcodes: behind every frame the encoder's rendering is iiv_render_rgb of the maps
    read back with iiv_encoder_get_state (and the model's); an encoder that renders and one that does not, on the same
    seeds, end in the same state and emit the same opcodes afterwards; a stream range past the end is refused."""
    import stream_batch
    import torch
    S = 2
    fm, fa = stream_batch.synth_frames_torch(S, 4, mode == R.DHGR, seed=17)
    pal = _palettes()["NTSC"]
    drawn, plain = H.seeded_batch(device_tables, mode, S), H.seeded_batch(device_tables, mode, S)
    ops = {id(drawn): [], id(plain): []}
    for f in range(3):
        seg = [(f, f & 1 if mode == R.DHGR else 0, 1, 40)]
        for b in (drawn, plain):
            ops[id(b)].append(b.enc.encode(fm, fa, seg).cpu().numpy())
        got = native.encoder_render(drawn.enc, pal)
        assert tuple(got.shape) == (S, 192, 560, 3)
        mem = np.stack([drawn.enc.get_state(native.STATE_MEM_MAIN, s) for s in range(S)])
        aux = np.stack([drawn.enc.get_state(native.STATE_MEM_AUX, s) for s in range(S)]) if mode == R.DHGR else np.zeros_like(mem)   # (an HGR encoder has no aux items)
        assert mem.any()
        again = native.render_rgb(mode, pal, torch.from_numpy(mem).cuda(), torch.from_numpy(aux).cuda() if mode == R.DHGR else None)
        assert torch.equal(got, again)
        want = R.render_rgb(mode, mem, aux, pal)
        assert (got.cpu().numpy() == want).all(), _first_difference(got.cpu().numpy(), want)
        assert torch.equal(drawn.screens_rgb(), got)                        # StreamBatch.screens_rgb: NTSC unless told otherwise
        one = native.encoder_render(drawn.enc, pal, first_stream=1, n_streams=1)
        assert torch.equal(one[0], got[1])
    # a range that is not inside the encoder's: refused, nothing written
    obuf, oview = guarded(S * FRAME, 64, 64, GUARD)
    hp = np.ascontiguousarray(pal).reshape(48)
    for first, count in ((1, 2), (2, 1), (-1, 1), (0, 3), (0, -1)):
        rc = native.lib().iiv_encoder_render(drawn.enc._h, first, count, native.hptr(hp), native.dptr(oview), native.stream_ptr())
        assert rc == native.ERR_INVALID, (first, count)
    assert native.lib().iiv_encoder_render(drawn.enc._h, 0, 1, native.hptr(hp), C.c_void_p(oview.data_ptr() + 8), native.stream_ptr()) == native.ERR_INVALID
    assert native.lib().iiv_encoder_render(drawn.enc._h, 2, 0, native.hptr(hp), native.dptr(oview), native.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (obuf.cpu().numpy() == GUARD).all()
    # the rendering changed nothing: same state, same opcodes from here on
    for b in (drawn, plain):
        ops[id(b)].append(b.enc.encode(fm, fa, [(3, 0, 1, 60)]).cpu().numpy())
        b.enc.check()
    for x, y in zip(ops[id(drawn)], ops[id(plain)]):
        assert (x == y).all()
    for name in [n for n in H.STATE_NAMES if mode == R.DHGR or "AUX" not in n]:
        for s in range(S):
            assert (drawn.enc.get_state(getattr(native, name), s) == plain.enc.get_state(getattr(native, name), s)).all(), name
    drawn.close()
    plain.close()


class _FG:
    input_frame_rate = 30


@pytest.mark.parametrize("mode", MODES)
def test_video_screen_rgb_and_screen_render_rgb(native, O, oracle_tables, mode):
    """The drop-in Video: screen_rgb() between and in the middle of generators is the rendering of the memory maps the Video
    shows (screen.render_rgb of them; the model's), and the opcodes around it stay the oracle's."""
    import palette
    import screen
    import torch
    import video
    import video_mode
    vm = video_mode.VideoMode.DHGR if mode == R.DHGR else video_mode.VideoMode.HGR
    frames = H.synth(mode, 2, 909)
    random.seed(31)
    np.random.seed(32)
    v = video.Video(_FG(), ticks_per_second=14700., mode=vm, palette=palette.Palette.NTSC)
    ov = O.Video(mode, oracle_tables.get(mode, 5), seed_py=31, seed_np=32)
    pal = palette.NTSCPalette.rgb_array()

    def shown():
        rgb = v.screen_rgb()
        assert tuple(rgb.shape) == (192, 560, 3) and rgb.is_cuda
        main = np.array(v.memory_map.page_offset)
        aux = np.array(v.aux_memory_map.page_offset) if mode == R.DHGR else np.zeros_like(main)
        assert (main == ov.memory(0)).all()
        tm, ta = torch.from_numpy(main[None]).cuda(), torch.from_numpy(aux[None]).cuda() if mode == R.DHGR else None
        assert torch.equal(screen.render_rgb(tm, ta, vm, palette.Palette.NTSC)[0], rgb)
        assert torch.equal(screen.render_rgb(tm, ta, mode, pal)[0], rgb)
        want = R.render_rgb(mode, main, aux, pal)
        assert (rgb.cpu().numpy() == want).all()
        return rgb

    got, want = [], []
    with contextlib.redirect_stdout(io.StringIO()):
        blank = shown()
        assert (blank.cpu().numpy() == pal[0]).all()
        for fi, ia, k in [(0, 0, 120), (1, 1 if mode == R.DHGR else 0, 80)]:
            Bitmap = screen.DHGRBitmap if mode == R.DHGR else screen.HGRBitmap
            kw = {"aux_memory": screen.MemoryMap(1, frames[fi, 1].copy())} if mode == R.DHGR else {}
            tgt = Bitmap(main_memory=screen.MemoryMap(1, frames[fi, 0].copy()), palette=palette.Palette.NTSC, **kw)
            gen = v.encode_frame(tgt, is_aux=bool(ia))
            ov.encode_frame(frames[fi, 0], frames[fi, 1] if mode == R.DHGR else None, ia)
            for part in (k // 2, k - k // 2):
                for _ in range(part):
                    page, content, offsets = next(gen)
                    got.append([page, content] + list(offsets))
                want.append(ov.next(part))
                assert not torch.equal(shown(), blank)        # in the middle of a generator, and behind it
            gen = None
    assert (np.array(got, np.uint8) == np.concatenate(want)).all()


def test_transcode_clip_preview(native, device_tables, tmp_path):
    """tools/transcode_clip.py --synthetic 4 --preview: an array (4, 192, 560, 3) whose last frame is the rendering of the screen
    the encoder ends on -- reproduced here with ONE encode call for the four frames, where the tool makes four --, and the
    .a2m bytes of a run without the option."""
    import frame_grabber
    import palette
    import stream_batch
    import torch
    import video_mode
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import transcode_clip
    tool = [sys.executable, os.path.join(ROOT, "tools", "transcode_clip.py"), "--synthetic", "4", "--seed", "3"]
    runs = [subprocess.Popen(tool + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)     # (side by side: two processes)
            for extra in (["--out", str(tmp_path / "a.a2m"), "--preview", str(tmp_path / "a.npy")], ["--out", str(tmp_path / "b.a2m")])]
    for r in runs:
        _, err = r.communicate(timeout=600)
        assert r.returncode == 0, err
    assert (tmp_path / "a.a2m").read_bytes() == (tmp_path / "b.a2m").read_bytes()
    shots = np.load(tmp_path / "a.npy")
    assert shots.shape == (4, 192, 560, 3) and shots.dtype == np.uint8
    assert all((shots[f] != shots[f + 1]).any() for f in range(3))
    grab = frame_grabber.ArrayFrameGrabber(transcode_clip.test_card(4), video_mode.VideoMode.DHGR, palette.Palette.NTSC,
                                           dither="diffusion", resize=True)
    main, aux = grab.memory_maps()
    table, store = device_tables.get(native.DHGR)
    batch = stream_batch.StreamBatch(native.DHGR, table, store, 1, seeds=[(3, 3)], dm=device_tables.dm[(native.DHGR, 5)],
                                     input_frame_rate=grab.input_frame_rate)
    batch.encode_frames(main[None], aux[None], 4)
    batch.enc.check()
    final = batch.screens_rgb(palette.Palette.NTSC).cpu().numpy()[0]
    assert (shots[3] == final).all()
    mem, am = batch.enc.get_state(native.STATE_MEM_MAIN), batch.enc.get_state(native.STATE_MEM_AUX)
    assert (final == R.render_rgb(R.DHGR, mem, am, palette.NTSCPalette.rgb_array())).all()
    batch.close()
