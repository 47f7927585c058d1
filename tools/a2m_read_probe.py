"""Probe: the .a2m reader's kernels alone (csrc/iiv_a2m_read.hip) -- opcodes/s of iiv_a2m_scan, iiv_a2m_decode and iiv_a2m_replay
(final snapshot; and 30 snapshots) on a device-resident batch of random DHGR streams of 14 699 opcodes (the length of the
reference-recorded movies of tests/golden/g7_movie.npz), next to iiv_emit_stream's rate writing those very streams and to the read
rate tools/hbm_stream measures in this session (run first, in a process of its own); the same for one stream alone; and replay
+ iiv_render_rgb of the batch against tests/a2m_model.py + tests/render_model.py on one of its streams (the sanity condition of
DESIGN.md 15: the batch on the device must take less time than the model takes for it).  HIP events around the calls, one
warm-up call, then several repetitions, every one printed.
    python tools/a2m_read_probe.py [streams] [repetitions] > profiles/a2m_read_probe.txt"""
import os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ii-vision_amd", "transcoder"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

S = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
R = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N = 14699
out = subprocess.run([os.path.join(ROOT, "tools", "hbm_stream")], capture_output=True, text=True, timeout=300).stdout
m = re.search(r"best: copy \(read \+ write bytes\) ([\d.]+) GB/s, read ([\d.]+) GB/s, write ([\d.]+) GB/s", out)
read_gbs = float(m.group(2)) if m else float("nan")
print("tools/hbm_stream, this session: %s" % (out.strip().splitlines()[-1] if out.strip() else "no output"), flush=True)

import numpy as np, torch
import _iiv_native as native, a2m, palette

addr = a2m.OpcodeAddresses.placeholder()
reader = native.A2mReaderHandle(addr.tick, addr.ack, addr.terminate)
pal = palette.NTSCPalette.rgb_array()
print("a2m_read_probe: %d opcodes per stream, %d repetitions, build %s" % (N, R, native.build_id()), flush=True)


def timed(name, call, n_streams, bytes_moved):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(R):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    best = min(ms)
    gbs = bytes_moved / (best * 1e-3) / 1e9
    print("%-34s %5d streams  best %8.3f ms (%s)  %9.1f M opcodes/s  %6.0f GB/s  share of the read rate %.3f" % (
        name, n_streams, best, " ".join("%.3f" % v for v in ms), n_streams * N / (best * 1e-3) / 1e6, gbs, gbs / read_gbs), flush=True)
    return best


for n_streams in (S, 1):
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    ops = torch.randint(0, 256, (n_streams, N, 6), dtype=torch.uint8, device="cuda", generator=g)
    ops[:, :, 0] = torch.randint(32, 64, (n_streams, N), dtype=torch.uint8, device="cuda", generator=g)
    ticks = (torch.randint(0, 32, (n_streams, N), device="cuda", generator=g) * 2 + 4).to(torch.uint8)
    data = a2m.emit_stream(native.DHGR, ops, ticks, addr)
    L = int(data.shape[1])
    lengths = torch.full((n_streams,), L, dtype=torch.int64, device="cuda")
    info = reader.scan(data, lengths)
    assert (info.cpu().numpy() == [0, 1, N, 0]).all()
    stream_bytes, op_bytes = n_streams * L, n_streams * N * 8
    timed("iiv_emit_stream (with its sync)", lambda: a2m.emit_stream(native.DHGR, ops, ticks, addr), n_streams, stream_bytes + n_streams * N * 7)
    timed("iiv_a2m_scan", lambda: reader.scan(data, lengths), n_streams, stream_bytes)
    timed("iiv_a2m_decode", lambda: reader.decode(data, info), n_streams, stream_bytes + op_bytes)
    t_final = timed("iiv_a2m_replay, final snapshot", lambda: reader.replay(data, info, 1 << 40, 1, 1), n_streams, stream_bytes + n_streams * 16384)
    if n_streams <= 1024:
        timed("iiv_a2m_replay, 30 snapshots", lambda: reader.replay(data, info, 490, 490, 30), n_streams, stream_bytes + n_streams * 30 * 16384)
    got = reader.decode(data, info)
    assert torch.equal(got[0][:, :N], ops) and torch.equal(got[1][:, :N], ticks)

    def replay_render():
        main, aux = reader.replay(data, info, 1 << 40, 1, 1)
        return native.render_rgb(native.DHGR, pal, main, aux)
    t_dev = timed("replay + iiv_render_rgb", replay_render, n_streams, stream_bytes + n_streams * (2 * 16384 + 192 * 560 * 3))
    if n_streams == S:
        import a2m_model, render_model
        one = data[0].cpu().numpy()
        t0 = time.perf_counter()
        mm, ma = a2m_model.replay(one, addr.tick, addr.ack, addr.terminate, 1 << 40, 1, 1)
        render_model.render_rgb(native.DHGR, mm, ma, pal)
        t_model = time.perf_counter() - t0
        main, aux = reader.replay(data, info, 1 << 40, 1, 1)
        assert np.array_equal(main[0, 0].cpu().numpy(), mm[0]) and np.array_equal(aux[0, 0].cpu().numpy(), ma[0])
        print("    the numpy model, ONE stream: %.1f ms; the device, all %d streams: %.3f ms (%.0f x faster than the model for the batch)" % (
            t_model * 1e3, n_streams, t_dev, t_model * 1e3 * n_streams / t_dev), flush=True)
    del ops, ticks, data
reader.close()
