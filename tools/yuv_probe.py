"""What taking 4:2:0 frames costs (csrc/iiv_resize.hip): batches of device-resident I420 frames at 640x480,
1280x720 and 1920x1080 resized to 280x192, HIP events around each call, one warm-up call and --reps repetitions, the median:

    fused      iiv_resize_frames_yuv420 on the planes (the conversion inside the horizontal pass)
    rgb        iiv_resize_frames on the RGB frames the same planes define (the resize as it was: the yardstick)
    separate   the alternative to fusing, where the public interface can express it (h, w <= 1024): the planes converted to RGB
               frames in memory -- iiv_resize_frames_yuv420 at the SAME size, which is the conversion kernel plus a copy pass, so
               an upper bound on a conversion kernel alone -- and then iiv_resize_frames

The three are timed alternately in one session, and the fused output is compared with the rgb output byte for byte at the
sizes timed.  Writes its lines to --out (profiles/yuv_probe.txt) and to stdout.

    python tools/yuv_probe.py [--frames 1024] [--reps 5] [--out profiles/yuv_probe.txt]

Kernel times: run it under rocprofv3 --kernel-trace --stats (a run of its own)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))

SIZES = [(480, 640), (720, 1280), (1080, 1920)]


def synth(torch, n, h, w, seed=1):
    """(y, u, v) planes made on the device: a drifting luma ramp with noise, two chroma gradients"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    y, u, v = (torch.empty(s, dtype=torch.uint8, device="cuda") for s in ((n, h, w), (n, ch, cw), (n, ch, cw)))
    for f0 in range(0, n, 64):
        k = min(64, n - f0)
        f = torch.arange(f0, f0 + k, device="cuda")[:, None, None]
        yy, xx = torch.arange(h, device="cuda")[None, :, None], torch.arange(w, device="cuda")[None, None, :]
        y[f0:f0 + k] = ((xx * 219 // w + yy // 8 + 2 * f) % 220 + 16 + torch.randint(-12, 13, (k, h, w), device="cuda", generator=g)).clamp(0, 255).to(torch.uint8)
        yy, xx = torch.arange(ch, device="cuda")[None, :, None], torch.arange(cw, device="cuda")[None, None, :]
        u[f0:f0 + k] = ((xx * 255 // cw + f) % 256 + 0 * yy).to(torch.uint8)
        v[f0:f0 + k] = ((yy * 255 // ch + 3 * f) % 256 + 0 * xx).to(torch.uint8)
    return y, u, v


def to_rgb(torch, y, u, v, matrix):
    """include/iivision.h f11 in torch integer arithmetic, 16 frames at a time -> uint8 (n, h, w, 3)"""
    y_off, ky, rv, gu, gv, bu = matrix
    n, h, w = y.shape
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    rows, cols = torch.arange(h, device="cuda") >> 1, torch.arange(w, device="cuda") >> 1
    for f0 in range(0, n, 16):
        c = (y[f0:f0 + 16].to(torch.int32) - y_off) * ky + 128
        d = u[f0:f0 + 16].to(torch.int32)[:, rows][:, :, cols] - 128
        e = v[f0:f0 + 16].to(torch.int32)[:, rows][:, :, cols] - 128
        out[f0:f0 + 16, ..., 0] = ((c + rv * e) >> 8).clamp(0, 255).to(torch.uint8)
        out[f0:f0 + 16, ..., 1] = ((c + gu * d + gv * e) >> 8).clamp(0, 255).to(torch.uint8)
        out[f0:f0 + 16, ..., 2] = ((c + bu * d) >> 8).clamp(0, 255).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_probe.txt"))
    a = ap.parse_args()
    import torch
    import _iiv_native as native
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("4:2:0 planes -> 280x192 on %s, build %s; %d device-resident frames, HIP events, 1 warm-up + %d repetitions, the median; matrix bt601" % (
        torch.cuda.get_device_name(0), native.build_id(), a.frames, a.reps))
    say("fused = iiv_resize_frames_yuv420 (I420 planes); rgb = iiv_resize_frames on the RGB frames of the same planes; separate = "
        "iiv_resize_frames_yuv420 at the same size (conversion kernel + copy pass) then iiv_resize_frames")
    m = native.YUV_MATRICES["bt601"]
    for (h, w) in SIZES:
        y, u, v = synth(torch, a.frames, h, w)
        rgb = to_rgb(torch, y, u, v, m)
        out_f = torch.empty((a.frames, 192, 280, 3), dtype=torch.uint8, device="cuda")
        out_r, out_s = torch.empty_like(out_f), torch.empty_like(out_f)
        separate = h <= 1024 and w <= 1024
        full = torch.empty((a.frames, h, w, 3), dtype=torch.uint8, device="cuda") if separate else None
        calls = {"fused": lambda: native.resize_frames_yuv420(y, u, v, out=out_f, matrix=m),
                 "rgb": lambda: native.resize_frames(rgb, out=out_r)}
        if separate:
            def two():
                native.resize_frames_yuv420(y, u, v, size=(h, w), out=full, matrix=m)
                native.resize_frames(full, out=out_s)
            calls["separate"] = two
        for c in calls.values():          # warm: tables, code objects, the scratch pool
            c()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_f, out_r)) and (not separate or bool(torch.equal(out_s, out_r)))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, c in calls.items():    # alternately: whatever else the box does hits all three alike
                e0.record()
                c()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
        say("%4dx%-4d n=%d: fused %.3f ms (min %.3f, max %.3f) = %.2f M frames/s, %.0f GB/s of planes | rgb %.3f ms (min %.3f, max %.3f) = "
            "%.2f M frames/s, %.0f GB/s of RGB | fused / rgb = %.3f%s | outputs equal: %s" % (
                w, h, a.frames, med["fused"], min(times["fused"]), max(times["fused"]), a.frames / med["fused"] / 1e3,
                a.frames * (h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)) / med["fused"] / 1e6, med["rgb"], min(times["rgb"]), max(times["rgb"]),
                a.frames / med["rgb"] / 1e3, a.frames * h * w * 3 / med["rgb"] / 1e6, med["fused"] / med["rgb"],
                " | separate %.3f ms (min %.3f, max %.3f), fused / separate = %.3f" % (
                    med["separate"], min(times["separate"]), max(times["separate"]), med["fused"] / med["separate"]) if separate
                else " | separate: not expressible (h or w > 1024)", same))
        del y, u, v, rgb, out_f, out_r, out_s, full, calls
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
