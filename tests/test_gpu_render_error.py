"""GPU: iiv_render_error / iiv_encoder_render_error (csrc/iiv_render_error.hip) -- the rendered screen against a reference
picture, nine exact sums per frame -- against tests/render_error_model.py, the numpy restatement of "f8: screen error" in
include/iivision.h on top of tests/render_model.py.  Every comparison is == on uint64:
  kernel = model   both modes x both reference widths x 0, 1, 2, 3, 5 frames, random screens (random hole bytes) and references,
                   the output pre-filled with 0xFF bytes; palettes of tests/ingest_model.py, NTSC, IIGS
  32-bit traps     white screen / black reference and blank screen / white reference: sums the model shows to be past 2^32
  zero and one     a reference rendered by iiv_render_rgb gives zeros; one byte of one dot changed gives its square at all levels
  independence     permuted frames give permuted sums; two calls back to back on one stream
  refusals         every invalid argument of the contract is IIV_ERR_INVALID, names the function and writes nothing
  encoder          iiv_encoder_render_error = iiv_render_error of the maps read back, and leaves the encoder as it was
  Python layer     screen.render_error, StreamBatch.screens_error, Video.screen_error, transcode_clip.py --quality"""
import contextlib
import ctypes as C
import io
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import encode_harness as H
import ingest_model
import render_error_model as E
import render_model as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [R.HGR, R.DHGR]
WIDTHS = [280, 560]
FILL = 0xFFFFFFFFFFFFFFFF

# 48 distinct bytes: a swapped channel or colour index changes a pixel
DISTINCT = ((np.arange(48) * 37 + 11) % 256).astype(np.uint8).reshape(16, 3)


def _random_case(n, width, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, 32, 256), dtype=np.uint8), rng.integers(0, 256, (n, 32, 256), dtype=np.uint8),
            rng.integers(0, 256, (n, 192, width, 3), dtype=np.uint8))


def _filled(torch, n):
    """(n, 3, 3) uint64 on the device, every byte 0xFF"""
    return torch.full((max(n, 1) * 72,), 0xFF, dtype=torch.uint8, device="cuda")[:n * 72].view(torch.uint64).view(n, 3, 3)


def _measure(native, mode, pal, main, aux, ref):
    import torch
    dm = torch.from_numpy(np.ascontiguousarray(main)).cuda()
    da = torch.from_numpy(np.ascontiguousarray(aux)).cuda() if mode == R.DHGR else None
    out = _filled(torch, len(main))
    got = native.render_error(mode, pal, dm, da, torch.from_numpy(np.ascontiguousarray(ref)).cuda(), out=out)
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu().numpy()
    assert got.shape == (len(main), 3, 3) and got.dtype == np.uint64
    return got


def _say(got, want):
    print("kernel\n%s\nmodel\n%s" % (got, want))
    return "kernel and model differ at (frame, level, channel) %s" % (np.argwhere(got != want)[:4].tolist(),)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_kernel_equals_model_on_random_screens(native, mode, width, n):
    """105 n wave runs, never a multiple of the four runs of a workgroup for these n; the output starts as 0xFF bytes: the
    call has to overwrite it; n = 0 leaves it alone."""
    import torch
    main, aux, ref = _random_case(n, width, 1000 * mode + 10 * n + width)
    if n == 0:
        out = _filled(torch, 1)
        m = torch.zeros((1, 32, 256), dtype=torch.uint8, device="cuda")
        r = torch.zeros((1, 192, width, 3), dtype=torch.uint8, device="cuda")
        pal = np.ascontiguousarray(DISTINCT).reshape(48)
        rc = native.lib().iiv_render_error(mode, native.hptr(pal), 0, native.dptr(m), native.dptr(m), native.dptr(r), width,
                                           native.dptr(out), native.stream_ptr())
        assert rc == 0
        assert tuple(native.render_error(mode, DISTINCT, m[:0], m[:0], r[:0]).shape) == (0, 3, 3)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == FILL).all()
        return
    got = _measure(native, mode, DISTINCT, main, aux, ref)
    want = E.render_error(mode, main, aux, DISTINCT, ref)
    assert (got == want).all(), _say(got, want)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_sums_past_32_bits(native, mode, width):
    """Every dot lit under a palette whose value 15 is white, against a black reference; a blank screen against a white one:
    the model's level-0 sums are past 2^32 (checked here), so a 32-bit accumulator anywhere cannot pass."""
    pal = DISTINCT.copy()
    pal[15] = (255, 255, 255)
    pal[0] = (0, 0, 0)
    lit = np.full((2, 32, 256), 0x7f if mode == R.DHGR else 0xff, np.uint8)
    blank = np.zeros((2, 32, 256), np.uint8)
    main = np.concatenate([lit, blank])
    ref = np.concatenate([np.zeros((2, 192, width, 3), np.uint8), np.full((2, 192, width, 3), 255, np.uint8)])
    want = E.render_error(mode, main, main, pal, ref)
    assert (want[:, 0, :] > np.uint64(2 ** 32)).all() and (want[:, 1, :] > want[:, 0, :]).all() and (want[:, 2, :] > want[:, 1, :]).all()
    assert want[2].tolist() == [[107520 * 255 ** 2] * 3, [26880 * 1020 ** 2] * 3, [6720 * 4080 ** 2] * 3]
    got = _measure(native, mode, pal, main, main, ref)
    assert (got == want).all(), _say(got, want)


@pytest.mark.parametrize("pal_name", list(ingest_model.PALETTES) + ["NTSC", "IIGS"])
def test_palettes(native, pal_name):
    import palette
    pal = (ingest_model.PALETTES[pal_name] if pal_name in ingest_model.PALETTES
           else {"NTSC": palette.NTSCPalette, "IIGS": palette.IIGSPalette}[pal_name].rgb_array())
    for mode in MODES:
        main, aux, ref = _random_case(1, 280 if mode == R.HGR else 560, 31 + mode)
        got = _measure(native, mode, pal, main, aux, ref)
        want = E.render_error(mode, main, aux, pal, ref)
        assert (got == want).all(), _say(got, want)


# (frame, y, x, channel) of the one byte that differs: a unit's last and first dot, a row's last and first, the first and the
# last dot of a frame, in the first and the last of three frames
ONE_DOT = [(0, 0, 0, 0), (0, 0, 15, 1), (0, 0, 16, 2), (0, 57, 559, 0), (0, 58, 0, 1), (0, 191, 559, 2), (2, 0, 0, 2), (2, 100, 303, 0),
           (2, 191, 559, 1), (1, 109, 400, 1)]


@pytest.mark.parametrize("mode", MODES)
def test_own_rendering_is_zero_and_one_changed_byte_is_its_square(native, mode):
    import torch
    main, aux, _ = _random_case(3, 560, 500 + mode)
    dm, da = torch.from_numpy(main).cuda(), torch.from_numpy(aux).cuda()
    shot = native.render_rgb(mode, DISTINCT, dm, da if mode == R.DHGR else None)
    got = native.render_error(mode, DISTINCT, dm, da, shot, out=_filled(torch, 3)).cpu().numpy()
    assert not got.any(), got
    refs, wants = [], []
    for i, (f, y, x, ch) in enumerate(ONE_DOT):
        ref = shot.clone()
        delta = 1 + 13 * i                                          # 1 .. 118: old + delta or old - delta is a byte
        old = int(ref[f, y, x, ch])
        new = old + delta if old + delta < 256 else old - delta
        assert 0 <= new < 256
        ref[f, y, x, ch] = new
        want = np.zeros((3, 3, 3), np.uint64)
        want[f, :, ch] = delta * delta                              # the same in the quad and the unit that hold the dot
        refs.append(ref)
        wants.append(want)
    out = _filled(torch, 3 * len(ONE_DOT))
    for i, ref in enumerate(refs):                                  # (all enqueued, then read together)
        native.render_error(mode, DISTINCT, dm, da, ref, out=out[3 * i:3 * i + 3])
    got = out.cpu().numpy().reshape(len(ONE_DOT), 3, 3, 3)
    for i, where in enumerate(ONE_DOT):
        assert (got[i] == wants[i]).all(), (where, got[i].tolist())


@pytest.mark.parametrize("mode", MODES)
def test_frames_are_independent_and_calls_queue(native, mode):
    """Permuting frames and references permutes the sums; two calls enqueued back to back on one stream into different
    outputs (different widths) are both right."""
    import torch
    n = 5
    main, aux, ref = _random_case(n, 560, 900 + mode)
    narrow = np.ascontiguousarray(ref[:, :, ::2])
    perm = np.array([3, 0, 4, 2, 1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dm, da, dr, dn = t(main), t(aux), t(ref), t(narrow)
    pm, pa, pr = t(main[perm]), t(aux[perm]), t(ref[perm])
    o1, o2, o3 = _filled(torch, n), _filled(torch, n), _filled(torch, n)
    native.render_error(mode, DISTINCT, dm, da, dr, out=o1)
    native.render_error(mode, DISTINCT, dm, da, dn, out=o2)
    native.render_error(mode, DISTINCT, pm, pa, pr, out=o3)
    g1, g2, g3 = o1.cpu().numpy(), o2.cpu().numpy(), o3.cpu().numpy()
    w1, w2 = E.render_error(mode, main, aux, DISTINCT, ref), E.render_error(mode, main, aux, DISTINCT, narrow)
    assert (g1 == w1).all(), _say(g1, w1)
    assert (g2 == w2).all(), _say(g2, w2)
    assert (g3 == w1[perm]).all() and (g1 != g2).any()


def test_refusals_write_nothing(native):
    import torch
    L = native.lib()
    n = 2
    main, aux, ref = _random_case(n, 560, 77)
    dm, da = torch.from_numpy(main).cuda(), torch.from_numpy(aux).cuda()
    dr = torch.from_numpy(ref).cuda()
    pal = np.ascontiguousarray(DISTINCT).reshape(48)
    out = _filled(torch, n + 1)
    st = native.stream_ptr()

    def call(mode, count, pm, pa, pr, width, po):
        return L.iiv_render_error(mode, native.hptr(pal), count, C.c_void_p(pm), C.c_void_p(pa), C.c_void_p(pr), width, C.c_void_p(po), st)

    m, a, r, o = dm.data_ptr(), da.data_ptr(), dr.data_ptr(), out.data_ptr()
    assert r % 16 == 0 and o % 8 == 0
    refused = {"mode 2": (2, n, m, a, r, 560, o), "mode -1": (-1, n, m, a, r, 560, o), "n < 0": (R.DHGR, -1, m, a, r, 560, o),
               "no main": (R.HGR, n, 0, a, r, 560, o), "DHGR without aux": (R.DHGR, n, m, 0, r, 560, o),
               "no reference": (R.HGR, n, m, a, 0, 560, o), "no output": (R.HGR, n, m, a, r, 560, 0),
               "width 0": (R.DHGR, n, m, a, r, 0, o), "width 140": (R.DHGR, n, m, a, r, 140, o), "width 281": (R.HGR, n, m, a, r, 281, o),
               "width 1120": (R.HGR, n, m, a, r, 1120, o), "main off by 4": (R.HGR, 1, m + 4, a, r, 560, o),
               "aux off by 4": (R.DHGR, 1, m, a + 4, r, 560, o), "reference off by 8": (R.DHGR, 1, m, a, r + 8, 560, o),
               "reference off by 1": (R.HGR, 1, m, a, r + 1, 280, o), "output off by 4": (R.DHGR, 1, m, a, r, 560, o + 4),
               "output off by 1": (R.HGR, 1, m, a, r, 280, o + 1)}
    for what, args in refused.items():
        assert call(*args) == native.ERR_INVALID, what
        assert b"iiv_render_error" in L.iiv_last_error(), what
    assert L.iiv_render_error(R.HGR, None, n, C.c_void_p(m), C.c_void_p(a), C.c_void_p(r), 560, C.c_void_p(o), st) == native.ERR_INVALID
    assert b"iiv_render_error" in L.iiv_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all()
    # HGR needs no aux (and does not look at a misaligned one); the output may sit at 8 bytes and no more
    want = E.render_error(R.HGR, main, None, DISTINCT, ref)
    assert call(R.HGR, n, m, 0, r, 560, o + 8) == 0
    assert out.data_ptr() % 16 == 0
    flat = out.cpu().numpy().reshape(-1)
    assert flat[0] == FILL and (flat[1:1 + 9 * n].reshape(n, 3, 3) == want).all() and (flat[1 + 9 * n:] == FILL).all()
    assert call(R.HGR, n, m, a + 4, r, 560, o) == 0
    assert (out.cpu().numpy().reshape(-1)[:9 * n].reshape(n, 3, 3) == want).all()


@pytest.mark.parametrize("mode", MODES)
def test_encoder_render_error(native, device_tables, mode):
    """Three streams, two frames of forty opcodes: behind each the encoder's sums -- the full range at width 560, the middle
    stream alone at width 280 -- are iiv_render_error's on the maps read back (and the model's); StreamBatch.screens_error is
    the same call; an encoder that measures and a twin that does not end in the same state and emit the same opcodes
    afterwards; ranges outside the encoder are refused and write nothing."""
    import palette
    import stream_batch
    import torch
    S = 3
    fm, fa = stream_batch.synth_frames_torch(S, 3, mode == R.DHGR, seed=17)
    pal = palette.NTSCPalette.rgb_array()
    _, _, ref = _random_case(S, 560, 60 + mode)
    narrow = np.ascontiguousarray(ref[:, :, 1::2])
    dref, dnarrow = torch.from_numpy(ref).cuda(), torch.from_numpy(narrow).cuda()
    measured, plain = H.seeded_batch(device_tables, mode, S), H.seeded_batch(device_tables, mode, S)
    ops = {id(measured): [], id(plain): []}
    for f in range(2):
        seg = [(f, f & 1 if mode == R.DHGR else 0, 1, 40)]
        for b in (measured, plain):
            ops[id(b)].append(b.enc.encode(fm, fa, seg).cpu().numpy())
        got = native.encoder_render_error(measured.enc, pal, dref, out=_filled(torch, S)).cpu().numpy()
        mid = native.encoder_render_error(measured.enc, pal, dnarrow[1:2], first_stream=1, n_streams=1, out=_filled(torch, 1)).cpu().numpy()
        mem = np.stack([measured.enc.get_state(native.STATE_MEM_MAIN, s) for s in range(S)])
        aux = np.stack([measured.enc.get_state(native.STATE_MEM_AUX, s) for s in range(S)]) if mode == R.DHGR else np.zeros_like(mem)
        assert mem.any()
        again = _measure(native, mode, pal, mem, aux, ref)
        assert (got == again).all(), _say(got, again)
        want = E.render_error(mode, mem, aux, pal, ref)
        assert (got == want).all(), _say(got, want)
        wmid = E.render_error(mode, mem[1:2], aux[1:2], pal, narrow[1:2])
        assert (mid == wmid).all(), _say(mid, wmid)
        assert (measured.screens_error(dref).cpu().numpy() == want).all()      # NTSC unless told otherwise
        assert (measured.screens_error(dref, palette.Palette.IIGS).cpu().numpy()
                == E.render_error(mode, mem, aux, palette.IIGSPalette.rgb_array(), ref)).all()
    out = _filled(torch, S)
    hp = np.ascontiguousarray(pal).reshape(48)
    L, h, st = native.lib(), measured.enc._h, native.stream_ptr()
    for first, count in ((1, 3), (3, 1), (-1, 1), (0, 4), (0, -1)):
        assert L.iiv_encoder_render_error(h, first, count, native.hptr(hp), native.dptr(dref), 560, native.dptr(out), st) == native.ERR_INVALID, (first, count)
        assert b"iiv_encoder_render_error" in L.iiv_last_error()
    r, o = dref.data_ptr(), out.data_ptr()
    for pr, width, po in ((r, 561, o), (r, 0, o), (r + 8, 560, o), (r, 560, o + 4), (0, 560, o), (r, 560, 0)):
        assert L.iiv_encoder_render_error(h, 0, 1, native.hptr(hp), C.c_void_p(pr), width, C.c_void_p(po), st) == native.ERR_INVALID, (pr - r, width, po - o)
        assert b"iiv_encoder_render_error" in L.iiv_last_error()
    assert L.iiv_encoder_render_error(h, 0, 1, None, C.c_void_p(r), 560, C.c_void_p(o), st) == native.ERR_INVALID
    assert L.iiv_encoder_render_error(None, 0, 1, native.hptr(hp), C.c_void_p(r), 560, C.c_void_p(o), st) == native.ERR_INVALID
    assert L.iiv_encoder_render_error(h, 3, 0, native.hptr(hp), C.c_void_p(r), 560, C.c_void_p(o), st) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all()
    # the measurement changed nothing: same state, same opcodes from here on
    for b in (measured, plain):
        ops[id(b)].append(b.enc.encode(fm, fa, [(2, 0, 1, 60)]).cpu().numpy())
        b.enc.check()
    for x, y in zip(ops[id(measured)], ops[id(plain)]):
        assert (x == y).all()
    for name in [n for n in H.STATE_NAMES if mode == R.DHGR or "AUX" not in n]:
        for s in range(S):
            assert (measured.enc.get_state(getattr(native, name), s) == plain.enc.get_state(getattr(native, name), s)).all(), name
    measured.close()
    plain.close()


class _FG:
    input_frame_rate = 30


@pytest.mark.parametrize("mode", MODES)
def test_video_screen_error_and_screen_render_error(native, O, oracle_tables, mode):
    """The drop-in Video: screen_error() in the middle of a generator is the model's sums of the memory maps the Video shows,
    screen.render_error of them agrees, and the opcodes around it stay the oracle's."""
    import palette
    import screen
    import torch
    import video
    import video_mode
    vm = video_mode.VideoMode.DHGR if mode == R.DHGR else video_mode.VideoMode.HGR
    frames = H.synth(mode, 1, 909)
    random.seed(31)
    np.random.seed(32)
    v = video.Video(_FG(), ticks_per_second=14700., mode=vm, palette=palette.Palette.NTSC)
    ov = O.Video(mode, oracle_tables.get(mode, 5), seed_py=31, seed_np=32)
    pal = palette.NTSCPalette.rgb_array()
    _, _, ref = _random_case(1, 280, 70 + mode)
    dref = torch.from_numpy(ref).cuda()

    def measured():
        got = v.screen_error(dref[0])
        assert tuple(got.shape) == (3, 3) and got.is_cuda and got.dtype == torch.uint64
        main = np.array(v.memory_map.page_offset)
        aux = np.array(v.aux_memory_map.page_offset) if mode == R.DHGR else np.zeros_like(main)
        want = E.render_error(mode, main[None], aux[None], pal, ref)
        assert (got.cpu().numpy() == want[0]).all()
        tm, ta = torch.from_numpy(main[None]).cuda(), torch.from_numpy(aux[None]).cuda() if mode == R.DHGR else None
        assert (screen.render_error(tm, ta, vm, palette.Palette.NTSC, dref).cpu().numpy() == want).all()
        assert (screen.render_error(tm, ta, mode, pal, dref).cpu().numpy() == want).all()
        per, overall = screen.psnr(got)
        mper, mall = E.psnr(want[0], 0)
        assert (per == mper).all() and overall == mall
        return want

    got, want = [], []
    with contextlib.redirect_stdout(io.StringIO()):
        blank = measured()
        Bitmap = screen.DHGRBitmap if mode == R.DHGR else screen.HGRBitmap
        kw = {"aux_memory": screen.MemoryMap(1, frames[0, 1].copy())} if mode == R.DHGR else {}
        tgt = Bitmap(main_memory=screen.MemoryMap(1, frames[0, 0].copy()), palette=palette.Palette.NTSC, **kw)
        gen = v.encode_frame(tgt, is_aux=False)
        ov.encode_frame(frames[0, 0], frames[0, 1] if mode == R.DHGR else None, 0)
        for part in (60, 60):
            for _ in range(part):
                page, content, offsets = next(gen)
                got.append([page, content] + list(offsets))
            want.append(ov.next(part))
            assert (measured() != blank).any()
        gen = None
    assert (np.array(got, np.uint8) == np.concatenate(want)).all()


def test_transcode_clip_quality(native, tmp_path):
    """tools/transcode_clip.py --synthetic 4 --quality: the .a2m bytes of a run without the option, and JSON sums equal to the
    model applied to the tool's own --preview pictures and the frames that went into the ingest (the test card, 280 wide)."""
    import screen
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import transcode_clip
    tool = [sys.executable, os.path.join(ROOT, "tools", "transcode_clip.py"), "--synthetic", "4", "--seed", "3"]
    runs = [subprocess.Popen(tool + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)     # (side by side: two processes)
            for extra in (["--out", str(tmp_path / "a.a2m"), "--preview", str(tmp_path / "a.npy"), "--quality", str(tmp_path / "q.json")],
                          ["--out", str(tmp_path / "b.a2m")])]
    for r in runs:
        _, err = r.communicate(timeout=600)
        assert r.returncode == 0, err
    assert (tmp_path / "a.a2m").read_bytes() == (tmp_path / "b.a2m").read_bytes()
    shots = np.load(tmp_path / "a.npy")
    assert shots.shape == (4, 192, 560, 3)
    with open(tmp_path / "q.json") as f:
        q = json.load(f)
    assert q["ref_width"] == 280 and len(q["frames"]) == 4
    want = E.error_sums_of_screens(shots, transcode_clip.test_card(4))
    assert [fr["sums"] for fr in q["frames"]] == want.tolist()
    assert want[:, 0].all()                                             # (a dithered card is never exact per dot)
    for level in range(3):
        assert [fr["psnr_db"][level] for fr in q["frames"]] == screen.psnr(want, level)[1].tolist()
