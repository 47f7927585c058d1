"""GPU: the .a2m reader (include/iivision.h section f9; csrc/iiv_a2m_read.hip) against the reference's recordings and the numpy
model (tests/a2m_model.py), byte for byte: scan, decode, replay to screen memory, the round trip through iiv_emit_stream, every
status, the encoder's own screen memory, the command-line tool, and the refusals."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import a2m_cases
import a2m_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G6 = ("HGR_a", "DHGR_a", "DHGR_b", "DHGR_c", "HGR_limit", "DHGR_empty")
G7 = ("DHGR_n1", "DHGR_n2", "HGR_n1", "HGR_n2", "DHGR_n2_audio_end")


@pytest.fixture(scope="module")
def addr(golden):
    import a2m
    g = golden.g6_a2m
    return a2m.OpcodeAddresses(g["tick_addr"], g["special_addr"][0], g["special_addr"][1], g["special_addr"][2])


@pytest.fixture(scope="module")
def reader(native, addr):
    import a2m
    r = a2m.A2mReader(addr)
    yield r
    r.close()


def _model_args(addr):
    return addr.tick, addr.ack, addr.terminate


def _emit(mode, ops, ticks, addr):
    import torch
    import a2m
    return a2m.emit_stream(mode, torch.from_numpy(ops[None]).cuda(), torch.from_numpy(ticks[None]).cuda(), addr)[0].cpu().numpy()


def test_scan_and_decode_of_the_emitter_recordings(reader, addr, golden):
    g = golden.g6_a2m
    streams = [g[t + "/stream"] for t in G6]
    assert sorted(set(len(s) for s in streams)) == [2048, 4096, 6144, 8192]
    info = reader.scan(streams)
    decoded = reader.decode(streams)
    for i, t in enumerate(G6):
        n = {"HGR_limit": 427, "DHGR_empty": 0}.get(t, len(g[t + "/ops"]))
        assert tuple(info[i]) == (M.OK, int(g[t + "/meta"][0]), n, 0) == M.scan(streams[i], *_model_args(addr)), t
        mode, ops, ticks, banks = decoded[i]
        m_mode, m_ops, m_ticks, m_banks = M.decode(streams[i], *_model_args(addr))
        assert mode == m_mode == int(g[t + "/meta"][0])
        assert np.array_equal(ops.cpu().numpy(), g[t + "/ops"][:n]) and np.array_equal(ops.cpu().numpy(), m_ops), t
        assert np.array_equal(ticks.cpu().numpy(), g[t + "/ticks"][:n]) and np.array_equal(ticks.cpu().numpy(), m_ticks), t
        assert np.array_equal(banks.cpu().numpy(), m_banks), t


def test_final_snapshot_is_the_reference_movies_screen_memory(reader, golden):
    g = golden.g7_movie
    streams = [g[t + "/stream"] for t in G7]
    assert sorted(set(len(s) for s in streams)) == [18432, 104448]
    info = reader.scan(streams)
    assert [int(v) for v in info[:, 0]] == [0] * 5 and [int(v) for v in info[:, 2]] == [14699] * 4 + [2527]
    main, aux = reader.replay(streams, first=1 << 60, every=1, n=1)
    main, aux = main.cpu().numpy(), aux.cpu().numpy()
    for i, t in enumerate(G7):
        assert int(info[i, 1]) == int(g[t + "/meta"][0])
        assert np.array_equal(main[i, 0], g[t + "/mem_main"]), t
        if int(info[i, 1]) == 1:
            assert np.array_equal(aux[i, 0], g[t + "/mem_aux"]), t
        else:
            assert not aux[i].any(), t


def test_snapshots_are_the_models_prefix_replays(reader, addr, golden):
    import torch
    stream = golden.g7_movie["DHGR_n1/stream"]
    main, aux = (t.cpu().numpy()[0] for t in reader.replay([stream], first=0, every=490, n=32))
    m_main, m_aux = M.replay(stream, *_model_args(addr), first=0, every=490, n=32)
    assert not main[0].any() and not aux[0].any()
    assert np.array_equal(main, m_main) and np.array_equal(aux, m_aux)
    assert 490 * 29 < 14699 <= 490 * 30 and np.array_equal(main[31], main[30]) and np.array_equal(aux[31], aux[30])
    assert not np.array_equal(main[30], main[29]) or not np.array_equal(aux[30], aux[29])
    rng = np.random.default_rng(11)
    init = rng.integers(0, 256, (2, 1, 32, 256), dtype=np.uint8)
    main, aux = (t.cpu().numpy()[0] for t in reader.replay([stream], first=0, every=490, n=32,
                                                           init=(torch.from_numpy(init[0]).cuda(), torch.from_numpy(init[1]).cuda())))
    m_main, m_aux = M.replay(stream, *_model_args(addr), first=0, every=490, n=32, init=(init[0, 0], init[1, 0]))
    assert np.array_equal(main[0], init[0, 0]) and np.array_equal(aux[0], init[1, 0])
    assert np.array_equal(main, m_main) and np.array_equal(aux, m_aux)


def test_collisions_keep_stream_order(reader, addr):
    """5 000 opcodes on one page whose offsets come from three values: every byte is hit thousands of times and most opcodes
    name an offset more than once -- the shape at which a store that is not ordered goes wrong"""
    rng = np.random.default_rng(3)
    ops, ticks = M.random_ops(rng, 5000, pages=(40, 41), offsets=(7, 8, 200))
    for mode in (0, 1):
        stream = _emit(mode, ops, ticks, addr)
        main, aux = (t.cpu().numpy()[0] for t in reader.replay([stream], first=100, every=100, n=50))
        m_main, m_aux = M.replay(stream, *_model_args(addr), first=100, every=100, n=50)
        assert np.array_equal(main, m_main) and np.array_equal(aux, m_aux), mode
        assert len({main[j].tobytes() + aux[j].tobytes() for j in range(50)}) > 40   # (the snapshots do differ)


def test_replay_across_many_folds_and_acks(reader, addr):
    rng = np.random.default_rng(4)
    ops, ticks = M.random_ops(rng, 100000)
    stream = _emit(1, ops, ticks, addr)
    assert len(M._acks_before(100000)) == 342 and 100000 > 24 * 4096   # ACKs after opcode 290 + 292 i; two dozen folds
    info = reader.scan([stream])
    assert tuple(info[0]) == (M.OK, 1, 100000, 0)
    n = 100000 // 7777 + 2
    main, aux = (t.cpu().numpy()[0] for t in reader.replay([stream], first=7777, every=7777, n=n))
    m_main, m_aux = M.replay(stream, *_model_args(addr), first=7777, every=7777, n=n)
    assert np.array_equal(main, m_main) and np.array_equal(aux, m_aux)


def test_sequence_restarts_at_every_fold(native, reader, addr):
    """2^24 + 50 opcodes: one more than a stamp's 24 sequence bits could count if the sequence ran on across folds.  Opcode k
    stores ((7 k + 3) ^ (k >> 8)) & 0xff at offset k & 0xff of page 32 (two opcodes at one offset differ), so the page's last writers are known in closed form; the window
    that holds opcode 2^24 begins 3096 opcodes before it and ends with the stream."""
    import torch
    import a2m
    n = (1 << 24) + 50
    k = torch.arange(n, device="cuda")
    ops = torch.empty((1, n, 6), dtype=torch.uint8, device="cuda")
    ops[0, :, 0] = 32
    ops[0, :, 1] = (((7 * k + 3) ^ (k >> 8)) & 0xff).to(torch.uint8)
    ops[0, :, 2:] = (k & 0xff).to(torch.uint8)[:, None]
    del k
    stream = a2m.emit_stream(0, ops, torch.full((1, n), 34, dtype=torch.uint8, device="cuda"), addr)
    del ops
    assert tuple(reader.scan(stream, [int(stream.shape[1])])[0]) == (M.OK, 0, n, 0)
    main, aux = reader.replay(stream, first=1000, every=1 << 40, n=2, lengths=[int(stream.shape[1])])
    last = n - 1 - ((n - 1 - np.arange(256)) % 256)            # the last opcode at each offset
    want = np.zeros((32, 256), np.uint8)
    want[0] = ((7 * last + 3) ^ (last >> 8)) & 0xff
    assert np.array_equal(main[0, 1].cpu().numpy(), want) and not aux.any()
    first = 999 - ((999 - np.arange(256)) % 256)
    assert np.array_equal(main[0, 0, 0].cpu().numpy(), (((7 * first + 3) ^ (first >> 8)) & 0xff).astype(np.uint8))


def test_round_trip_and_retarget(reader, addr, golden):
    import a2m
    g = golden.g6_a2m
    for t in G6:   # (HGR_limit, cut by max_bytes_out at 427 opcodes, is those 427 opcodes' whole stream)
        stream = g[t + "/stream"]
        mode, ops, ticks, _ = reader.decode([stream])[0]
        assert np.array_equal(a2m.emit_stream(mode, ops[None], ticks[None], addr)[0].cpu().numpy(), stream), t

    new = a2m.OpcodeAddresses.placeholder()
    new_reader = a2m.A2mReader(new)
    for t in ("HGR_a", "DHGR_a"):
        stream = g[t + "/stream"]
        moved = a2m.retarget(stream, addr, new).cpu().numpy()
        assert len(moved) == len(stream) and not np.array_equal(moved, stream)
        n = len(g[t + "/ops"])
        assert tuple(new_reader.scan([moved])[0]) == (M.OK, int(g[t + "/meta"][0]), n, 0)
        assert tuple(reader.scan([moved])[0]) == (M.BAD_ADDRESS, int(g[t + "/meta"][0]), 0, 7)
        a, b = reader.decode([stream])[0], new_reader.decode([moved])[0]
        assert a[0] == b[0] and all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a[1:], b[1:]))
    new_reader.close()


def test_every_status_in_one_batch(reader, addr, golden):
    import a2m
    cases = a2m_cases.broken_streams(golden.g6_a2m)
    info = reader.scan([c[1] for c in cases])
    for i, (name, b, want) in enumerate(cases):
        assert tuple(int(v) for v in info[i]) == want == M.scan(b, *_model_args(addr)), name
    # the opcodes a broken stream still has, and what strict reading says of it
    decoded = reader.decode([c[1] for c in cases], strict=False)
    for (name, b, want), (mode, ops, ticks, banks) in zip(cases, decoded):
        m = M.decode(b, *_model_args(addr))
        assert len(ops) == want[2] and np.array_equal(ops.cpu().numpy(), m[1]) and np.array_equal(banks.cpu().numpy(), m[3]), name
    with pytest.raises(ValueError, match=r"stream 1 is BAD_LENGTH at byte 0") as e:
        reader.decode([c[1] for c in cases])
    assert isinstance(e.value, a2m.A2mStreamError) and (e.value.stream, e.value.status, e.value.position) == (1, "BAD_LENGTH", 0)
    with pytest.raises(ValueError, match=r"stream 0 is BAD_ACK at byte 2046"):
        reader.replay([cases[9][1]])
    assert cases[9][0] == "bank byte 0x56"


def test_bank_comes_from_the_ack_byte(reader, addr, golden):
    """a stream whose ACKs all carry 0x55: every opcode behind the first ACK is in bank 1, in decode and in replay"""
    b = golden.g6_a2m["DHGR_a/stream"].copy()
    for p in (2046, 4094, 6142):
        b[p] = 0x55
    assert tuple(reader.scan([b])[0]) == (M.OK, 1, 1000, 0)
    banks = reader.decode([b])[0][3].cpu().numpy()
    assert not banks[:291].any() and banks[291:].all()
    main, aux = (t.cpu().numpy()[0] for t in reader.replay([b], first=1000))
    m_main, m_aux = M.replay(b, *_model_args(addr), first=1000, every=1, n=1)
    assert np.array_equal(main, m_main) and np.array_equal(aux, m_aux)


def test_replay_of_an_encoders_stream_is_the_encoders_screen_memory(native, reader, addr, device_tables):
    import torch
    import a2m
    import stream_batch
    t, s = device_tables.get(1)
    fm, fa = stream_batch.synth_frames_torch(2, 20, True, seed=21)
    b = stream_batch.StreamBatch(1, t, s, 2, seeds=[(1, 1), (2, 2)], dm=device_tables.dm[(1, 5)])
    ops, _ = b.encode_frames(fm, fa, 20)
    b.enc.check()
    ticks = torch.full((2, ops.shape[1]), 34, dtype=torch.uint8, device="cuda")
    streams = a2m.emit_stream(1, ops, ticks, addr)
    lengths = [int(streams.shape[1])] * 2
    assert [int(v) for v in reader.scan(streams, lengths)[:, 2]] == [int(ops.shape[1])] * 2
    main, aux = reader.replay(streams, first=1 << 40, lengths=lengths)
    for i in range(2):
        assert np.array_equal(main[i, 0].cpu().numpy(), b.enc.get_state(native.STATE_MEM_MAIN, i))
        assert np.array_equal(aux[i, 0].cpu().numpy(), b.enc.get_state(native.STATE_MEM_AUX, i))
    b.close()


def test_tool_previews_scores_and_checks(native, tmp_path):
    import a2m
    import palette
    import render_error_model
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))

    def run(tool, *args):
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)] + [str(x) for x in args], capture_output=True, text=True,
                              env=env, timeout=300)
    clip, shots = tmp_path / "clip.a2m", tmp_path / "a.npy"
    out = run("transcode_clip.py", "--synthetic", 4, "--out", clip, "--preview", shots)
    assert out.returncode == 0, out.stderr
    want = np.load(shots)
    data = np.fromfile(clip, dtype=np.uint8)
    ref = want[-1:, :, ::-1].copy()   # any picture will do as a reference: the last screen, mirrored
    np.save(tmp_path / "ref.npy", ref)
    out = run("play_a2m.py", clip, "--every", 1 << 40, "--preview", tmp_path / "b.npy", "--ref", tmp_path / "ref.npy", "--quality",
              tmp_path / "q.json", "--check")
    assert out.returncode == 0 and ": OK, mode DHGR" in out.stdout, out.stdout + out.stderr
    got = np.load(tmp_path / "b.npy")
    assert got.shape == (1, 192, 560, 3) and np.array_equal(got[0], want[-1])
    r = a2m.A2mReader(a2m.OpcodeAddresses.placeholder())
    main, aux = (t.cpu().numpy()[0] for t in r.replay([data], first=1 << 40))
    r.close()
    sums = render_error_model.render_error(1, main, aux, palette.palette_class(palette.Palette.NTSC).rgb_array(), ref)
    q = json.load(open(tmp_path / "q.json"))
    assert len(q["frames"]) == 1 and np.array_equal(np.array(q["frames"][0]["sums"], dtype=np.uint64), sums[0])
    data[2] ^= 0x40   # (a byte the format fixes; a flipped content byte is another movie, not a broken stream)
    data.tofile(tmp_path / "bad.a2m")
    out = run("play_a2m.py", tmp_path / "bad.a2m", "--check")
    assert out.returncode != 0 and ": OK" not in out.stdout, out.stdout + out.stderr


def test_refusals_write_nothing(native, addr, golden):
    import ctypes as C
    import torch
    L = native.lib()
    h = native.A2mReaderHandle(addr.tick, addr.ack, addr.terminate)
    stream = golden.g6_a2m["DHGR_b/stream"]
    data = torch.from_numpy(stream[None].copy()).cuda()
    lengths = torch.tensor([len(stream)], dtype=torch.int64, device="cuda")
    good = h.scan(data, lengths)
    n = native.a2m_max_ops(len(stream))
    info = torch.full((2, 4), -7, dtype=torch.int64, device="cuda")
    ops = torch.full((n * 6 + 8,), 0xAA, dtype=torch.uint8, device="cuda")
    ticks, banks = ops.clone()[:n + 8], ops.clone()[:n + 8]
    main, aux = torch.full((2, 8192), 0xAA, dtype=torch.uint8, device="cuda"), torch.full((2, 8192), 0xAA, dtype=torch.uint8, device="cuda")
    p, st, null = native.dptr, native.stream_ptr(), C.c_void_p(0)
    stride = len(stream)
    odd = C.c_void_p(info.data_ptr() + 4)
    refused = [
        L.iiv_a2m_scan(null, 1, p(data), stride, p(lengths), p(info), st),
        L.iiv_a2m_scan(h._h, 1, null, stride, p(lengths), p(info), st),
        L.iiv_a2m_scan(h._h, 1, p(data), stride, null, p(info), st),
        L.iiv_a2m_scan(h._h, 1, p(data), stride, p(lengths), null, st),
        L.iiv_a2m_scan(h._h, -1, p(data), stride, p(lengths), p(info), st),
        L.iiv_a2m_scan(h._h, 1, p(data), 2047, p(lengths), p(info), st),
        L.iiv_a2m_scan(h._h, 1, p(data), stride, p(lengths), odd, st),
        L.iiv_a2m_decode(null, 1, p(data), stride, p(good), p(ops), n * 6, p(ticks), p(banks), n, st),
        L.iiv_a2m_decode(h._h, 1, p(data), stride, p(good), null, n * 6, p(ticks), p(banks), n, st),
        L.iiv_a2m_decode(h._h, 1, p(data), stride, p(good), p(ops), n * 6, null, p(banks), n, st),
        L.iiv_a2m_decode(h._h, 1, p(data), stride, p(good), p(ops), n * 6, p(ticks), null, n, st),
        L.iiv_a2m_decode(h._h, 1, p(data), stride, p(good), p(ops), n * 6 - 1, p(ticks), p(banks), n, st),
        L.iiv_a2m_decode(h._h, 1, p(data), stride, p(good), p(ops), n * 6, p(ticks), p(banks), n - 1, st),
        L.iiv_a2m_decode(h._h, 1, p(data), 100, p(good), p(ops), n * 6, p(ticks), p(banks), n, st),
        L.iiv_a2m_replay(null, 1, p(data), stride, p(good), 0, 1, 1, null, null, p(main), p(aux), st),
        L.iiv_a2m_replay(h._h, 1, p(data), stride, null, 0, 1, 1, null, null, p(main), p(aux), st),
        L.iiv_a2m_replay(h._h, 1, p(data), stride, p(good), -1, 1, 1, null, null, p(main), p(aux), st),
        L.iiv_a2m_replay(h._h, 1, p(data), stride, p(good), 0, 0, 1, null, null, p(main), p(aux), st),
        L.iiv_a2m_replay(h._h, 1, p(data), stride, p(good), 0, 1, 0, null, null, p(main), p(aux), st),
        L.iiv_a2m_replay(h._h, 1, p(data), stride, p(good), 0, 1, 1, null, null, null, p(aux), st),
        L.iiv_a2m_replay(h._h, 1, p(data), stride, p(good), 0, 1, 1, null, null, C.c_void_p(main.data_ptr() + 4), p(aux), st),
        L.iiv_a2m_replay(h._h, 1, p(data), stride, p(good), 0, 1, 1, C.c_void_p(main.data_ptr() + 1), null, p(main), p(aux), st),
        L.iiv_a2m_replay(h._h, 1, p(data), 2000, p(good), 0, 1, 1, null, null, p(main), p(aux), st),
    ]
    assert refused == [native.ERR_INVALID] * len(refused)
    # n_streams == 0 succeeds and writes nothing
    assert L.iiv_a2m_scan(h._h, 0, p(data), stride, p(lengths), p(info), st) == 0
    assert L.iiv_a2m_decode(h._h, 0, p(data), stride, p(good), p(ops), n * 6, p(ticks), p(banks), n, st) == 0
    assert L.iiv_a2m_replay(h._h, 0, p(data), stride, p(good), 0, 1, 1, null, null, p(main), p(aux), st) == 0
    torch.cuda.synchronize()
    assert (info == -7).all() and (ops == 0xAA).all() and (ticks == 0xAA).all() and (banks == 0xAA).all()
    assert (main == 0xAA).all() and (aux == 0xAA).all()
    # and decode leaves the bytes past n_ops alone
    assert L.iiv_a2m_decode(h._h, 1, p(data), stride, p(good), p(ops), n * 6, p(ticks), p(banks), n, st) == 0
    torch.cuda.synchronize()
    assert int(good[0, 2]) == 291 and (ops[291 * 6:] == 0xAA).all() and (ticks[291:] == 0xAA).all() and (banks[291:] == 0xAA).all()
    assert np.array_equal(ops[:291 * 6].cpu().numpy().reshape(291, 6), golden.g6_a2m["DHGR_b/ops"])
    h.close()
