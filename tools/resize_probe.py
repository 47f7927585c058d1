"""The resize's rate on the device (csrc/iiv_resize.hip): batches of device-resident frames at 640x480, 1280x720 and
1920x1080 resized to 280x192 (frame_grabber.py:75,100), timed with HIP events around iiv_resize_frames, against the read
floor (source bytes / bench.py's HBM_MEASURED_READ_GBS) and against Pillow's LANCZOS on this host's CPU at 1 and 16
threads; then one tools/transcode_clip.py run on a 640x480 clip.

    python tools/resize_probe.py [--frames 1024] [--reps 5] [--no-pillow] [--no-clip]

Kernel times: run it under rocprofv3 --kernel-trace --stats."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))
import numpy as np  # noqa: E402

HBM_MEASURED_READ_GBS = 7070.0   # bench.py: what plain kernels read from HBM on this part (tools/hbm_stream.hip)
SIZES = [(480, 640), (720, 1280), (1080, 1920)]


def synth(torch, n, h, w, seed=1):
    """gradients, bars and noise made on the device"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    y = torch.arange(h, device="cuda")[:, None]
    x = torch.arange(w, device="cuda")[None, :]
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    for f0 in range(0, n, 64):
        k = min(64, n - f0)
        f = torch.arange(f0, f0 + k, device="cuda")[:, None, None]
        base = torch.stack([(x * 255 // w + f) % 256 + 0 * y, (y * 255 // h + 0 * x + 0 * f), ((x + 3 * f) // 40 % 2) * 255 + 0 * y],
                           -1)
        noise = torch.randint(-24, 25, (k, h, w, 3), device="cuda", generator=g)
        out[f0:f0 + k] = (base + noise).clamp(0, 255).to(torch.uint8)
    return out


def pillow_rate(frames, threads):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    imgs = [Image.fromarray(f) for f in frames]

    def one(im):
        return im.resize((280, 192), resample=Image.LANCZOS)
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, imgs[:threads]))                 # warm
        t0 = time.perf_counter()
        list(ex.map(one, imgs))
        return len(imgs) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-pillow", action="store_true")
    ap.add_argument("--no-clip", action="store_true")
    a = ap.parse_args()
    import torch
    import _iiv_native as native
    try:
        import PIL
        pil = None if a.no_pillow else PIL.__version__
    except ImportError:
        pil = None
    print("resize -> 280x192 on %s, build %s; read floor = source bytes / %.0f GB/s; Pillow %s on the host's CPU" % (
        torch.cuda.get_device_name(0), native.build_id(), HBM_MEASURED_READ_GBS, pil or "not measured"))
    for (h, w) in SIZES:
        src = synth(torch, a.frames, h, w)
        out = torch.empty((a.frames, 192, 280, 3), dtype=torch.uint8, device="cuda")
        native.resize_frames(src, out=out)                # warm: tables, code objects, the scratch pool
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(a.reps):
            e0.record()
            native.resize_frames(src, out=out)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / 1e3)
        t = min(times)
        floor = a.frames * h * w * 3 / (HBM_MEASURED_READ_GBS * 1e9)
        line = "%4dx%-4d n=%d: %.3f ms (median %.3f, max %.3f) = %.2f M frames/s, %.0f GB/s of source; read floor %.3f ms -> %.2f of it" % (
            w, h, a.frames, t * 1e3, sorted(times)[len(times) // 2] * 1e3, max(times) * 1e3, a.frames / t / 1e6, a.frames * h * w * 3 / t / 1e9,
            floor * 1e3, floor / t)
        if pil:
            host = src[:48].cpu().numpy()
            line += "; Pillow %.0f frames/s at 1 thread, %.0f at 16" % (pillow_rate(host[:16], 1), pillow_rate(host, 16))
        print(line, flush=True)
        del src, out
    if not a.no_clip:
        with tempfile.TemporaryDirectory() as d:
            clip = synth(torch, 150, 480, 640, seed=4).cpu().numpy()
            np.save(os.path.join(d, "clip.npy"), clip)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "transcode_clip.py"), "--frames",
                                os.path.join(d, "clip.npy"), "--out", os.path.join(d, "clip.a2m")],
                               capture_output=True, text=True, timeout=900)
            print("transcode_clip.py on a 150-frame 640x480 clip:", " / ".join(
                l for l in r.stdout.strip().splitlines()), "(exit %d)" % r.returncode)
            if r.returncode:
                print(r.stderr[-2000:])


if __name__ == "__main__":
    main()
