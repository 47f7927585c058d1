"""Probe: iiv_render_rgb alone -- frames/s of the preview kernel (csrc/iiv_render.hip) in both modes on a device-resident
batch of picture-like screens (the memory maps iiv_frames_to_memory_maps makes of stream_batch.synth_rgb_torch), HIP events
around the calls, one warm-up call, then several timed repetitions (every one printed: the spread is the noise), and the
same through iiv_encoder_render's strided view (the maps one encoder state apart) for a smaller batch.
    python tools/render_probe.py [frames per call] [repetitions] [--stream]
The kernel only streams, so its floor is (bytes written + bytes read) over what the box's HBM streams with plain kernels:
bench.py's HBM_MEASURED_COPY_GBS (a run of tools/hbm_stream, profiles/r04_hbm_stream.txt), or, with --stream, the figures
tools/hbm_stream measures in this very session (run first, in a process of its own).  share = floor time / measured time."""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))
sys.path.insert(0, ROOT)

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if len(args) > 0 else 8192
R = int(args[1]) if len(args) > 1 else 5
session = None
if "--stream" in sys.argv:
    out = subprocess.run([os.path.join(ROOT, "tools", "hbm_stream")], capture_output=True, text=True, timeout=300).stdout
    m = re.search(r"best: copy \(read \+ write bytes\) ([\d.]+) GB/s, read ([\d.]+) GB/s, write ([\d.]+) GB/s", out)
    session = tuple(float(v) for v in m.groups()) if m else None
    print("tools/hbm_stream, this session: %s" % (out.strip().splitlines()[-1] if out.strip() else "no output"), flush=True)

import numpy as np, torch
import bench
import _iiv_native as native, palette, stream_batch

FRAME_OUT = 192 * 560 * 3
copy_gbs = session[0] if session else bench.HBM_MEASURED_COPY_GBS
write_gbs = session[2] if session else None
pal = palette.NTSCPalette.rgb_array()
clips = 64
rgb = stream_batch.synth_rgb_torch(clips, max(N // clips, 1), seed=3).view(-1, 192, 280, 3)
n = int(rgb.shape[0])
out = torch.empty((n, 192, 560, 3), dtype=torch.uint8, device="cuda")
print("render_probe: %d frames per call (%.2f GB written), %d repetitions, build %s; floor: copy %.0f GB/s (%s)%s" % (
    n, n * FRAME_OUT / 1e9, R, native.build_id(), copy_gbs, "tools/hbm_stream in this session" if session else "bench.HBM_MEASURED_COPY_GBS",
    ", write alone %.0f GB/s" % write_gbs if write_gbs else ""), flush=True)


def timed(name, call, frames, in_bytes):
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
    gbs = frames * (FRAME_OUT + in_bytes) / (best * 1e-3) / 1e9
    print("%-34s %7d frames  best %.3f ms (%s)  %.2f M frames/s  %.0f GB/s  share of the floor %.2f%s" % (
        name, frames, best, " ".join("%.3f" % v for v in ms), frames / (best * 1e-3) / 1e6, gbs, gbs / copy_gbs,
        "  (of write alone %.2f)" % (gbs / write_gbs) if write_gbs else ""), flush=True)


for mode, name in ((native.DHGR, "DHGR"), (native.HGR, "HGR")):
    main, aux = native.frames_to_memory_maps(mode, pal, rgb, native.DITHER_DIFFUSION)
    timed("iiv_render_rgb %s" % name, lambda: native.render_rgb(mode, pal, main, aux, out=out), n, 16384 if mode == native.DHGR else 8192)
    # the same kernel over an encoder's own screens: the streams' states lie ~300 KB apart
    S = min(n, 1024)
    dm = palette.diff_matrix(palette.Palette.NTSC)
    enc = native.Encoder(mode, native.build_table(mode, dm, True), native.build_store_table(mode, dm), S, dm=dm)
    enc.set_state_all(native.STATE_MEM_MAIN, main[:S].cpu().numpy())
    if mode == native.DHGR:
        enc.set_state_all(native.STATE_MEM_AUX, aux[:S].cpu().numpy())
    timed("iiv_encoder_render %s" % name, lambda: native.encoder_render(enc, pal, out=out[:S]), S, 16384 if mode == native.DHGR else 8192)
    assert torch.equal(out[:S], native.render_rgb(mode, pal, main[:S], aux[:S] if aux is not None else None))
    enc.close()
    del main, aux
