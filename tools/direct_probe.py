"""Probe: iiv_frames_to_memory_maps_direct alone -- frames/s on device-resident picture-like RGB
(stream_batch.synth_rgb_torch), both modes, beside iiv_frames_to_memory_maps' ordered and error-diffusion kernels on the same
frames.  HIP events, one warm-up call and five repetitions each; the median is printed.
    python tools/direct_probe.py [frames per call]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ii-vision_amd", "transcoder"))
import numpy as np, torch
import _iiv_native as native, stream_batch, palette

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
pal = palette.NTSCPalette.rgb_array()
clips = 64
rgb = stream_batch.synth_rgb_torch(clips, N // clips, seed=3).view(-1, 192, 280, 3)
n = int(rgb.shape[0])
main = torch.empty((n, 32, 256), dtype=torch.uint8, device="cuda")
aux = torch.empty_like(main)
print("%d picture-like frames, 280 wide, NTSC palette (build %s): median of five, HIP events" % (n, native.build_id()))
for mode_name, mode in (("DHGR", native.DHGR), ("HGR", native.HGR)):
    calls = [("direct 0", lambda: native.frames_to_memory_maps_direct(mode, pal, rgb, 0, out=(main, aux))),
             ("direct 32", lambda: native.frames_to_memory_maps_direct(mode, pal, rgb, 32, out=(main, aux))),
             ("direct 0 + cost", lambda: native.frames_to_memory_maps_direct(mode, pal, rgb, 0, cost=True, out=(main, aux))),
             ("ordered 32", lambda: native.frames_to_memory_maps(mode, pal, rgb, 32, out=(main, aux))),
             ("diffusion", lambda: native.frames_to_memory_maps(mode, pal, rgb, native.DITHER_DIFFUSION, out=(main, aux)))]
    for name, call in calls:
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        dt = float(np.median(ms)) * 1e-3
        print("%-5s %-16s %9.3f ms  %8.3f M frames/s   (five: %s)" % (mode_name, name, dt * 1e3, n / dt / 1e6,
                                                                      " ".join("%.3f" % m for m in ms)), flush=True)
