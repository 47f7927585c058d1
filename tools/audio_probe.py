"""The audio track's rate on the device (csrc/iiv_audio.hip): PCM synthesised on the GPU for a bench-like batch (default
14336 streams x 33 s of 44.1 kHz stereo), ticks timed with HIP events for 131072-frame decode blocks (the reference's
read_data(128 * 1024), audio.py:98) and for 2048-frame blocks, for a batch of streams of distinct lengths (with the device's
free memory before and after it), and the normalisation (audio.py:60-78) of a smaller batch.

    python tools/audio_probe.py [--streams 14336] [--seconds 33] [--reps 3]

Prints one JSON line per measurement: G ticks/s against the 5 G ticks/s target (about 3x the 1.7 G ticks/s the encode
consumes at 3.5 M DHGR frames/s and 490 ticks a frame).  Kernel times: run it under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))


def synth(torch, n_streams, n_frames, channels, seed=1):
    """a sine per stream, a slow chirp and noise, int16 interleaved, made on the device chunk by chunk"""
    pcm = torch.empty((n_streams, n_frames * channels), dtype=torch.int16, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.arange(n_frames, device="cuda", dtype=torch.float32) / 44100.0
    for s0 in range(0, n_streams, 256):
        s1 = min(n_streams, s0 + 256)
        f = 200.0 + 30.0 * torch.arange(s0, s1, device="cuda", dtype=torch.float32)[:, None]
        x = 8000 * torch.sin(2 * 3.14159265 * f * t) + 3000 * torch.sin(2 * 3.14159265 * (50 * t + 300 * t * t))
        x = x[:, :, None] + torch.randn((s1 - s0, n_frames, channels), device="cuda", generator=g) * 1500
        pcm[s0:s1] = x.clamp(-32768, 32767).to(torch.int16).reshape(s1 - s0, -1)
    return pcm


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=14336)
    ap.add_argument("--seconds", type=float, default=33.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--norm-streams", type=int, default=512)
    ap.add_argument("--distinct-streams", type=int, default=2048)
    a = ap.parse_args()
    import torch
    import _iiv_native as native
    n_frames = int(a.seconds * a.rate)
    free, _ = torch.cuda.mem_get_info()
    per_stream = n_frames * a.channels * 2 + native.audio_tick_count(n_frames, a.rate, 14700, 2048)
    streams = min(a.streams, int((free - (8 << 30)) // per_stream))   # (the FFT work buffers: 2 GiB, and slack)
    pcm = synth(torch, streams, n_frames, a.channels)
    torch.cuda.synchronize()
    for block in (131072, 2048):
        n_ticks = native.audio_tick_count(n_frames, a.rate, 14700, block)
        out = torch.empty((streams, n_ticks), dtype=torch.uint8, device="cuda")
        native.audio_ticks(pcm, n_frames, a.channels, a.rate, 3.0, block_frames=block, out=out)   # warm-up: tables, code
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            native.audio_ticks(pcm, n_frames, a.channels, a.rate, 3.0, block_frames=block, out=out)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / 1e3)
        t = min(times)
        total = streams * n_ticks
        print(json.dumps({"stage": "ticks", "block_frames": block, "streams": streams, "seconds_of_audio": a.seconds,
                          "channels": a.channels, "rate": a.rate, "ticks": total, "s": round(t, 4), "s_all": [round(x, 4) for x in times],
                          "g_ticks_per_s": round(total / t / 1e9, 3), "target_g_ticks_per_s": 5.0,
                          "pcm_gb_per_s": round(streams * n_frames * a.channels * 2 / t / 1e9, 1)}), flush=True)
        del out
    # streams of distinct lengths: every stream's last block is a length of its own (its own Bluestein tables and launches);
    # the call's device memory is freed behind it, so the free memory after it equals the free memory before
    nd = min(streams, a.distinct_streams)
    lens = n_frames - 37 * torch.arange(nd).numpy()
    n_ticks = max(native.audio_tick_count(int(n), a.rate, 14700, 131072) for n in lens)
    out = torch.empty((nd, n_ticks), dtype=torch.uint8, device="cuda")
    native.audio_ticks(pcm[:8], lens[:8], a.channels, a.rate, 3.0, out=out[:8])   # warm-up
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _, counts = native.audio_ticks(pcm[:nd], lens, a.channels, a.rate, 3.0, out=out)
    e1.record()
    e1.synchronize()
    t = e0.elapsed_time(e1) / 1e3
    torch.cuda.empty_cache()
    free1 = torch.cuda.mem_get_info()[0]
    print(json.dumps({"stage": "ticks_distinct_lengths", "block_frames": 131072, "streams": nd, "distinct_last_blocks": nd,
                      "ticks": int(counts.sum()), "s": round(t, 4), "g_ticks_per_s": round(int(counts.sum()) / t / 1e9, 3),
                      "device_free_mib_before": free0 >> 20, "device_free_mib_after": free1 >> 20}), flush=True)
    del out
    ns = min(a.norm_streams, streams)
    native.audio_normalization(pcm[:1], n_frames, a.channels, a.rate)   # warm-up
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    norms = native.audio_normalization(pcm[:ns], n_frames, a.channels, a.rate)
    e1.record()
    e1.synchronize()
    t = e0.elapsed_time(e1) / 1e3
    print(json.dumps({"stage": "normalization", "streams": ns, "prefix_frames": native.audio_prefix_frames(n_frames, a.channels),
                      "s": round(t, 4), "ms_per_stream": round(t / ns * 1e3, 3), "norm_min": float(norms.min()),
                      "norm_max": float(norms.max())}), flush=True)


if __name__ == "__main__":
    main()
