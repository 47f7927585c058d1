"""Probe: iiv_frames_to_memory_maps_mono alone -- frames/s of the ordered-dither and error-diffusion kernels on
picture-like synthetic RGB (stream_batch.synth_rgb_torch, at one pixel per dot), device-resident frames, HIP events around
the calls, one warm-up call per dither, then several timed repetitions (every one printed: the spread is the noise).
    python tools/mono_probe.py [frames per call] [mode: DHGR|HGR] [repetitions]
The colour conversion's rate on the frames these were made from: tools/ingest_probe.py with the same frame count, in the
same session (profiles/mono_probe.txt holds both)."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ii-vision_amd", "transcoder"))
import numpy as np, torch
import _iiv_native as native, stream_batch

N = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
mode = native.HGR if (len(sys.argv) > 2 and sys.argv[2] == "HGR") else native.DHGR
R = int(sys.argv[3]) if len(sys.argv) > 3 else 5
W = native.MONO_SIZE[mode][1]
clips = 256
src = stream_batch.synth_rgb_torch(clips, max(N // clips, 1), seed=3).view(-1, 192, 280, 3)
rgb = src.repeat_interleave(W // 280, dim=2).contiguous() if W != 280 else src
n = int(rgb.shape[0])
main = torch.empty((n, 32, 256), dtype=torch.uint8, device="cuda")
aux = torch.empty_like(main)
print("mono_probe: %s, %d frames of 192 x %d per call, %d repetitions, build %s, chunk %s" % (
    "DHGR" if mode == native.DHGR else "HGR", n, W, R, native.build_id(), os.environ.get("IIV_EXP_MONO_CHUNK", "default")), flush=True)


def timed(name, call, in_bytes):
    call()                                   # warm-up: code objects, the memory pool's first growth
    torch.cuda.synchronize()
    ms = []
    for _ in range(R):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    best, med = min(ms), float(np.median(ms))
    out_bytes = 16384 if mode == native.DHGR else 8192
    print("%-22s median %8.3f ms = %6.2f M frames/s, %5.0f GB/s in+out   (best %.3f ms; all: %s)" % (
        name, med, n / med / 1e3, n * (in_bytes + out_bytes) / med / 1e6, best, " ".join("%.3f" % m for m in ms)), flush=True)


for name, d in (("mono none", 0), ("mono ordered 32", 32), ("mono diffusion", native.DITHER_DIFFUSION)):
    timed(name, lambda: native.frames_to_memory_maps_mono(mode, rgb, d, out=(main, aux)), 192 * W * 3)
