"""Probe: iiv_render_error alone -- frames/s of the screen-error kernel (csrc/iiv_render_error.hip) in both modes and at both
reference widths on a device-resident batch of picture-like screens (the memory maps iiv_frames_to_memory_maps makes of
stream_batch.synth_rgb_torch) against the pictures they were made of, HIP events around the calls, one warm-up call, then
several timed repetitions (every one printed: the spread is the noise); the same through iiv_encoder_render_error's
strided view for a smaller batch; and what a user had before: iiv_render_rgb to HBM, then a torch subtraction, squaring and
summation per frame and channel over the same frames (level 0 only: the dot sums).
    python tools/render_error_probe.py [frames per call] [repetitions] [--stream]
The kernel only reads, so its floor is the bytes read over what the box's HBM reads with a plain kernel: with --stream the
read rate tools/hbm_stream measures in this very session (run first, in a process of its own), else the copy rate of
bench.HBM_MEASURED_COPY_GBS.  share = achieved GB/s over that rate; the aim is 0.5 at width 560."""
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

read_gbs = session[1] if session else bench.HBM_MEASURED_COPY_GBS
pal = palette.NTSCPalette.rgb_array()
clips = 64
rgb280 = stream_batch.synth_rgb_torch(clips, max(N // clips, 1), seed=3).view(-1, 192, 280, 3).contiguous()
n = int(rgb280.shape[0])
rgb560 = rgb280.repeat_interleave(2, dim=2).contiguous()       # the same pictures at one pixel per dot
sums = torch.empty((n, 3, 3), dtype=torch.uint64, device="cuda")
print("render_error_probe: %d frames per call, %d repetitions, build %s; yardstick: %.0f GB/s (%s)" % (
    n, R, native.build_id(), read_gbs, "read rate of tools/hbm_stream in this session" if session else "bench.HBM_MEASURED_COPY_GBS"), flush=True)


def timed(name, call, frames, bytes_per_frame):
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
    gbs = frames * bytes_per_frame / (best * 1e-3) / 1e9
    print("%-40s %7d frames  best %.3f ms (%s)  %.2f M frames/s  %.0f GB/s  share of the read rate %.2f" % (
        name, frames, best, " ".join("%.3f" % v for v in ms), frames / (best * 1e-3) / 1e6, gbs, gbs / read_gbs), flush=True)
    return best


for mode, name in ((native.DHGR, "DHGR"), (native.HGR, "HGR")):
    main, aux = native.frames_to_memory_maps(mode, pal, rgb280, native.DITHER_DIFFUSION)
    maps = 16384 if mode == native.DHGR else 8192
    fused = {}
    for width, ref in ((560, rgb560), (280, rgb280)):
        fused[width] = timed("iiv_render_error %s width %d" % (name, width),
                             lambda: native.render_error(mode, pal, main, aux, ref, out=sums), n, 192 * width * 3 + maps + 72)
    # what there was before: the screen to HBM, then torch over it (level 0 only)
    shot = torch.empty((n, 192, 560, 3), dtype=torch.uint8, device="cuda")
    chunk = min(n, 512)                                        # (the int32 differences of a chunk: 1.3 GB at 512 frames)

    def unfused():
        native.render_rgb(mode, pal, main, aux, out=shot)
        res = []
        for i in range(0, n, chunk):
            d = shot[i:i + chunk].to(torch.int32) - rgb560[i:i + chunk].to(torch.int32)
            res.append((d * d).sum(dim=(1, 2), dtype=torch.int64))
        return torch.cat(res)

    t = timed("iiv_render_rgb + torch, %s width 560" % name, unfused, n, 2 * 192 * 560 * 3 + maps)
    got = native.render_error(mode, pal, main, aux, rgb560, out=sums).cpu().numpy()
    assert (got[:, 0, :].astype(np.int64) == unfused().cpu().numpy()).all()
    print("    fused / unfused at width 560, level 0 only: %.1f x faster" % (t / fused[560]), flush=True)
    del shot
    # the same kernel over an encoder's own screens: the streams' states lie ~300 KB apart
    S = min(n, 1024)
    dm = palette.diff_matrix(palette.Palette.NTSC)
    enc = native.Encoder(mode, native.build_table(mode, dm, True), native.build_store_table(mode, dm), S, dm=dm)
    enc.set_state_all(native.STATE_MEM_MAIN, main[:S].cpu().numpy())
    if mode == native.DHGR:
        enc.set_state_all(native.STATE_MEM_AUX, aux[:S].cpu().numpy())
    timed("iiv_encoder_render_error %s width 560" % name, lambda: native.encoder_render_error(enc, pal, rgb560[:S], out=sums[:S]), S,
          192 * 560 * 3 + maps + 72)
    assert (sums[:S].cpu().numpy() == got[:S]).all()
    enc.close()
    del main, aux
