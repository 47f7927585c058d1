"""Probe: iiv_frames_to_memory_maps_diffused alone -- frames/s of every named error-diffusion kernel
(frame_grabber.DIFFUSION_KERNELS, csrc/iiv_diffuse.hip) in both modes, and of the existing IIV_DITHER_DIFFUSION kernel
(csrc/iiv_ingest.hip) on the same frames in the same session: the yardstick.  Device-resident picture-like synthetic RGB
(stream_batch.synth_rgb_torch), HIP events around each call, one warm-up call per kernel, the median of five calls (every
one printed: the spread is the noise).
    python tools/diffusion_kernels_probe.py [frames per call] [repetitions]
What the encoder consumes is bench.py's `value` of the same session (profiles/diffusion_kernels_probe.txt holds both)."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ii-vision_amd", "transcoder"))
import numpy as np, torch
import _iiv_native as native, frame_grabber, palette, stream_batch

N = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
R = int(sys.argv[2]) if len(sys.argv) > 2 else 5
pal = palette.NTSCPalette.rgb_array()
clips = 256
rgb = stream_batch.synth_rgb_torch(clips, max(N // clips, 1), seed=3).view(-1, 192, 280, 3)
n = int(rgb.shape[0])
main = torch.empty((n, 32, 256), dtype=torch.uint8, device="cuda")
aux = torch.empty_like(main)
print("diffusion_kernels_probe: %d frames of 192 x 280 per call, %d repetitions, build %s" % (n, R, native.build_id()), flush=True)


def timed(call):
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
    return float(np.median(ms)), ms


for mode, mode_name in ((native.DHGR, "DHGR"), (native.HGR, "HGR")):
    base, ms = timed(lambda: native.frames_to_memory_maps(mode, pal, rgb, native.DITHER_DIFFUSION, out=(main, aux)))
    print("%-4s %-28s median %8.3f ms = %6.2f M frames/s   1.00 of it   (all: %s)" % (
        mode_name, "IIV_DITHER_DIFFUSION (old)", base, n / base / 1e3, " ".join("%.3f" % m for m in ms)), flush=True)
    for name, (w, d) in frame_grabber.DIFFUSION_KERNELS.items():
        rows = sum(1 for r in w[1:] if any(r))
        med, ms = timed(lambda: native.frames_to_memory_maps_diffused(mode, pal, rgb, w, d, out=(main, aux)))
        print("%-4s %-28s median %8.3f ms = %6.2f M frames/s   %.2f of it   (all: %s)" % (
            mode_name, "%s (%d row%s below)" % (name, rows, "" if rows == 1 else "s"), med, n / med / 1e3, base / med,
            " ".join("%.3f" % m for m in ms)), flush=True)
