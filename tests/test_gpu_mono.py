"""GPU: mono playback mode -- csrc/iiv_mono.hip against tests/mono_model.py byte for byte, the tables and the
encoder under the mono cost matrix against the oracle, and the mode through frame_grabber / StreamBatch / video.Video /
tools/transcode_clip.py against the oracle driven with the model's frames and the oracle's dm_mono tables."""
import contextlib
import io
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import mono_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [M.DHGR, M.HGR]
DITHERS = [0, 32, 255, M.DITHER_DIFFUSION]

_base, _maps, _otab = {}, {}, {}


def base_frames(mode):
    """structured frames, uniform noise, black / white / primaries / checkerboard / steep ramps: 13 frames per mode"""
    if mode not in _base:
        _base[mode] = np.ascontiguousarray(np.concatenate([M.structured_frames(mode, 3), M.noise_frames(mode, 1), M.corner_frames(mode)]))
    return _base[mode]


def model_maps(mode, dither):
    """the model's memory maps of base_frames(mode): computed once, shared, never written to"""
    if (mode, dither) not in _maps:
        main, aux = M.frames_to_memory_maps(mode, base_frames(mode), dither)
        main.setflags(write=False)
        if aux is not None:
            aux.setflags(write=False)
        _maps[(mode, dither)] = (main, aux)
    return _maps[(mode, dither)]


def oracle_table(O, mode):
    if mode not in _otab:
        _otab[mode] = O.build_table(mode, M.dm_mono(), symmetric=True)
    return _otab[mode]


@pytest.mark.parametrize("dither", DITHERS)
@pytest.mark.parametrize("mode", MODES)
def test_kernel_equals_model(native, mode, dither):
    """Byte for byte, for frame counts that are no multiple of the frames a workgroup takes (4) and one past a chunk of
    the error diffusion (2048 frames): the frames of a longer batch are the base frames over and over."""
    import torch
    rgb = torch.from_numpy(base_frames(mode)).cuda()
    em, ea = model_maps(mode, dither)
    em_d = torch.from_numpy(np.array(em)).cuda()
    ea_d = torch.from_numpy(np.array(ea)).cuda() if ea is not None else None
    counts = [1, 3, 13, 65] + ([2049] if dither == M.DITHER_DIFFUSION else [])
    for n in counts:
        idx = torch.arange(n, device="cuda") % len(rgb)
        main, aux = native.frames_to_memory_maps_mono(mode, rgb[idx].contiguous(), dither)
        assert main.shape == (n, 32, 256) and (aux is None) == (mode == M.HGR)
        bad = (main != em_d[idx]).reshape(n, -1).any(dim=1).nonzero().flatten().tolist()
        assert not bad, ("main", mode, dither, n, bad[:8])
        if mode == M.DHGR:
            bad = (aux != ea_d[idx]).reshape(n, -1).any(dim=1).nonzero().flatten().tolist()
            assert not bad, ("aux", mode, dither, n, bad[:8])


def test_bad_arguments_are_refused(native):
    import torch
    rgb = torch.zeros((2, 192, 560, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        native.frames_to_memory_maps_mono(M.HGR, rgb)                       # HGR takes 280 dots
    with pytest.raises(ValueError):
        native.frames_to_memory_maps_mono(M.DHGR, rgb[:, :, :280])
    with pytest.raises(native.IIVError):
        native.frames_to_memory_maps_mono(M.DHGR, rgb, 257)
    with pytest.raises(native.IIVError):
        native.frames_to_memory_maps_mono(M.DHGR, rgb, -1)
    main = torch.zeros((2, 32, 256), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        native.frames_to_memory_maps_mono(M.DHGR, rgb, 0, out=(main, None))
    L = native.lib()
    args = (2, native.dptr(rgb), 0, native.dptr(main), native.dptr(main), native.stream_ptr())
    assert L.iiv_frames_to_memory_maps_mono(7, *args) == native.ERR_INVALID
    odd = (2, native.C.c_void_p(rgb.data_ptr() + 2), 0, native.dptr(main), native.dptr(main), native.stream_ptr())
    assert L.iiv_frames_to_memory_maps_mono(M.DHGR, *odd) == native.ERR_INVALID
    odd = (2, native.dptr(rgb), 0, native.C.c_void_p(main.data_ptr() + 4), native.dptr(main), native.stream_ptr())
    assert L.iiv_frames_to_memory_maps_mono(M.DHGR, *odd) == native.ERR_INVALID
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", MODES)
def test_writes_into_a_batch_slice_asynchronously(native, mode):
    """out=: straight into a (streams, frames, 32, 256) slice of a batch's target frames, several calls back to back on one
    stream without a host synchronisation; the buffers start as 0xff, so an unwritten byte -- a hole -- shows."""
    import torch
    dev = torch.from_numpy(base_frames(mode)[:12]).cuda()
    main = torch.full((6, 4, 32, 256), 255, dtype=torch.uint8, device="cuda")
    aux = torch.full((6, 4, 32, 256), 255, dtype=torch.uint8, device="cuda") if mode == M.DHGR else None
    for dither, s0 in ((32, 0), (M.DITHER_DIFFUSION, 3)):      # streams 0..2 ordered, 3..5 diffusion
        native.frames_to_memory_maps_mono(mode, dev, dither, out=(main[s0:s0 + 3], aux[s0:s0 + 3] if aux is not None else None))
    torch.cuda.synchronize()
    for s0, dither in ((0, 32), (3, M.DITHER_DIFFUSION)):
        em, ea = model_maps(mode, dither)
        assert np.array_equal(main[s0:s0 + 3].cpu().numpy().reshape(12, 32, 256), em[:12]), (mode, dither)
        if mode == M.DHGR:
            assert np.array_equal(aux[s0:s0 + 3].cpu().numpy().reshape(12, 32, 256), ea[:12]), (mode, dither)


@pytest.mark.parametrize("mode", MODES)
def test_tables_and_fast_kernels_under_the_mono_matrix(native, O, mode):
    """build_table / build_store_table with dm_mono equal the oracle's entry for entry, the narrow form of the store table
    is exact, and an encoder created with dm = dm_mono takes every fast greedy kernel -- and gives the oracle's opcodes."""
    import palette
    import stream_batch
    import torch
    dm = palette.MonoPalette.diff_matrix()
    assert np.array_equal(dm, M.dm_mono())
    table = native.build_table(mode, dm, True)
    store = native.build_store_table(mode, dm)
    otab = oracle_table(O, mode)
    assert np.array_equal(native.table_to_numpy(table), otab)
    # the store table is a gather from the table (S[o][content][m] = table[o][(poke(m, content) << bits) + m]): from the oracle's
    otab_d = torch.from_numpy(otab.view(np.int16)).cuda()
    ostore = torch.empty_like(store)
    native.check(native.lib().iiv_store_table_from_table(mode, native.dptr(otab_d), native.dptr(ostore), native.stream_ptr()))
    assert torch.equal(store, ostore)
    del ostore, otab_d
    _, n_bad = native.build_narrow_store_table(mode, dm, store)
    assert n_bad == 0
    main, aux = model_maps(mode, M.DITHER_DIFFUSION)
    fm = torch.from_numpy(np.array(main[:2])).cuda()[None].contiguous()
    fa = torch.from_numpy(np.array(aux[:2])).cuda()[None].contiguous() if aux is not None else None
    want = None
    for kernel in (True, "team", "shared", "plain"):
        b = stream_batch.StreamBatch(mode, table, store, 1, seeds=[(5, 6)], dm=dm)
        b.enc.set_greedy_kernel(kernel)       # raises if the encoder were left with the dense-table workgroup kernel
        b.enc.profile(True)
        ops, segs = b.encode_frames(fm, fa, 2)
        b.enc.check()
        forms = b.enc.launch_forms()
        assert forms["workgroup"] == 0 and forms["plain"] + forms["shared"] + forms["team"] > 0, (kernel, forms)
        if kernel == "team":
            assert forms["team"] > 0, forms
        if want is None:
            v = O.Video(mode, otab, seed_py=5, seed_np=6)
            want = []
            for (f, ia, restart, k) in segs:
                if restart:
                    v.encode_frame(main[f], aux[f] if aux is not None else None, ia)
                want.append(v.next(k))
            want = np.concatenate(want)
        assert np.array_equal(ops.cpu().numpy()[0], want), kernel
        b.close()


@pytest.mark.parametrize("mode", MODES)
def test_frame_grabber_feeds_stream_batch(native, O, mode):
    """ArrayFrameGrabber(palette=MONO) -> StreamBatch, Movie pacing, two streams (error diffusion / ordered dither 32) of
    twenty frames: opcodes, final memory maps and both MT19937 positions equal the oracle driven with the model's frames
    and the oracle's dm_mono table."""
    import frame_grabber
    import palette
    import stream_batch
    import torch
    from video_mode import VideoMode
    vm = VideoMode.DHGR if mode == M.DHGR else VideoMode.HGR
    n = 20
    clips = [M.structured_frames(mode, n, seed=3), M.structured_frames(mode, n, seed=4)[::-1].copy()]
    dithers = ["diffusion", 32]
    mains, auxs, want_maps = [], [], []
    for rgb, d in zip(clips, dithers):
        fg = frame_grabber.ArrayFrameGrabber(rgb, vm, palette.Palette.MONO, dither=d, batch=7)
        m, a = fg.memory_maps()
        mains.append(m)
        auxs.append(a)
        em, ea = M.frames_to_memory_maps(mode, rgb, M.DITHER_DIFFUSION if d == "diffusion" else d)
        want_maps.append((em, ea))
        assert np.array_equal(m.cpu().numpy(), em) and (ea is None or np.array_equal(a.cpu().numpy(), ea))
    got = list(fg.frames())                                   # the host form, in batches of 7
    assert len(got) == n and all(np.array_equal(got[i][0].page_offset, want_maps[1][0][i]) for i in range(n))
    assert all((g[1] is None) if mode == M.HGR else np.array_equal(g[1].page_offset, want_maps[1][1][i]) for i, g in enumerate(got))
    dm = palette.diff_matrix(palette.Palette.MONO)
    table, store = native.build_table(mode, dm, True), native.build_store_table(mode, dm)
    b = stream_batch.StreamBatch(mode, table, store, 2, seeds=[(3, 4), (5, 6)], dm=dm)
    ops, segs = b.encode_frames(torch.stack(mains), torch.stack(auxs) if mode == M.DHGR else None, n)
    b.enc.check()
    ops = ops.cpu().numpy()
    otab = oracle_table(O, mode)
    for s, (sp, sn) in enumerate([(3, 4), (5, 6)]):
        em, ea = want_maps[s]
        v = O.Video(mode, otab, seed_py=sp, seed_np=sn)
        exp = []
        for (f, ia, restart, k) in segs:
            if restart:
                v.encode_frame(em[f], ea[f] if ea is not None else None, ia)
            exp.append(v.next(k))
        assert np.array_equal(ops[s], np.concatenate(exp)), (mode, s)
        st = b.enc.get_video_state(s)
        assert np.array_equal(st.array("mem_main", np.uint8, (32, 256)), v.memory(0))
        if mode == M.DHGR:
            assert np.array_equal(st.array("mem_aux", np.uint8, (32, 256)), v.memory(1))
        assert np.array_equal(st.array("rng_py", np.uint32, (625,)), v.rng_py().state_words())
        assert np.array_equal(st.array("rng_np", np.uint32, (625,)), v.rng_np().state_words())
    b.close()


def test_frame_grabber_resizes_to_the_dot_grid(native):
    """resize=True: frames of another size are resized to one pixel per dot first (the resize's own model says to what)."""
    import frame_grabber
    import palette
    import resize_model
    from video_mode import VideoMode
    src = np.random.default_rng(8).integers(0, 256, (2, 100, 210, 3), dtype=np.uint8)
    for mode, vm in ((M.DHGR, VideoMode.DHGR), (M.HGR, VideoMode.HGR)):
        fg = frame_grabber.ArrayFrameGrabber(src, vm, palette.Palette.MONO, dither="diffusion", resize=True)
        m, a = fg.memory_maps()
        rs = np.stack([resize_model.resize(f, size=(192, M.width(mode))) for f in src])
        em, ea = M.frames_to_memory_maps(mode, rs, M.DITHER_DIFFUSION)
        assert np.array_equal(m.cpu().numpy(), em) and (ea is None or np.array_equal(a.cpu().numpy(), ea))


class _FG:
    input_frame_rate = 30


@pytest.mark.parametrize("mode", MODES)
def test_video_drop_in_takes_the_mono_palette(native, O, mode):
    """video.Video(palette=Palette.MONO), driven generator by generator as movie.py drives it over twenty frames: the
    opcodes, the final memory maps and both global MT19937 positions equal the oracle's."""
    import ctypes as C
    import frame_grabber
    import palette
    import screen
    import stream_batch
    import video
    from video_mode import VideoMode
    vm = VideoMode.DHGR if mode == M.DHGR else VideoMode.HGR
    n = 20
    rgb = M.structured_frames(mode, n, seed=9)
    maps = list(frame_grabber.ArrayFrameGrabber(rgb, vm, palette.Palette.MONO, dither="diffusion").frames())
    em, ea = M.frames_to_memory_maps(mode, rgb, M.DITHER_DIFFUSION)
    random.seed(21)
    np.random.seed(22)
    v = video.Video(_FG(), ticks_per_second=14700., mode=vm, palette=palette.Palette.MONO)
    ov = O.Video(mode, oracle_table(O, mode), seed_py=21, seed_np=22)
    got, want, prev = [], [], None
    with contextlib.redirect_stdout(io.StringIO()):
        for (f, ia, _, k) in stream_batch.MovieClock(mode == M.DHGR).segments(n):
            assert np.array_equal(maps[f][0].page_offset, em[f])
            if mode == M.DHGR:
                tgt = screen.DHGRBitmap(main_memory=maps[f][0], aux_memory=maps[f][1], palette=palette.Palette.MONO)
            else:
                tgt = screen.HGRBitmap(main_memory=maps[f][0], palette=palette.Palette.MONO)
            gen = v.encode_frame(tgt, is_aux=bool(ia), budget=k)
            if f != prev:                                     # movie.py:96
                v.out_of_work = {True: False, False: False}
                ov.reset_out_of_work()
                prev = f
            for _ in range(k):
                page, content, offsets = next(gen)
                got.append([page, content] + list(offsets))
            gen = None
            ov.encode_frame(em[f], ea[f] if ea is not None else None, int(ia))
            want.append(ov.next(k))
    assert np.array_equal(np.array(got, np.uint8), np.concatenate(want))
    assert np.array_equal(v.memory_map.page_offset, ov.memory(0))
    if mode == M.DHGR:
        assert np.array_equal(v.aux_memory_map.page_offset, ov.memory(1))
    L = O.lib()
    rp, rn = ov.rng_py(), ov.rng_np()
    assert [random.getrandbits(8) for _ in range(4)] == [L.orc_py_getrandbits8(C.byref(rp)) for _ in range(4)]
    assert np.random.randint(0, 256, size=4).tolist() == [L.orc_np_randint256(C.byref(rn)) for _ in range(4)]


@pytest.mark.parametrize("mode_name", ["DHGR", "HGR"])
def test_transcode_clip_mono_equals_the_oracle_chain(tmp_path, O, mode_name):
    """tools/transcode_clip.py --synthetic 30 --palette MONO writes the bytes the same chain gives through the model and the
    oracle (encode restatement, emit restatement)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import stream_batch
    import transcode_clip
    n = 30
    out = tmp_path / "clip.a2m"
    args = [sys.executable, os.path.join(ROOT, "tools", "transcode_clip.py"), "--synthetic", str(n), "--out", str(out),
            "--mode", mode_name, "--palette", "MONO", "--seed", "7", "--tick", "20"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer(out.read_bytes(), np.uint8)
    mode = M.DHGR if mode_name == "DHGR" else M.HGR
    rgb = transcode_clip.test_card(n, M.width(mode))
    assert rgb.shape == (n, 192, M.width(mode), 3)
    em, ea = M.frames_to_memory_maps(mode, rgb, M.DITHER_DIFFUSION)
    v = O.Video(mode, oracle_table(O, mode), seed_py=7, seed_np=7)
    ops = []
    for (fr, ia, restart, k) in stream_batch.MovieClock(mode == M.DHGR).segments(n):
        if restart:
            v.encode_frame(em[fr], ea[fr] if ea is not None else None, ia)
        ops.append(v.next(k))
    ops = np.concatenate(ops)
    tick_addr = (0x8000 + 16 * np.arange(1024)).astype(np.uint16)
    exp = O.emit_stream(mode, ops, np.full(len(ops), 20, np.uint8), tick_addr, 0xc000, 0xc100)
    assert len(got) == len(exp) and len(got) % 2048 == 0
    assert (got == exp).all()
