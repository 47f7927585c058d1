"""The fitted resize's rate on the device (csrc/iiv_resize.hip, include/iivision.h f12): batches of device-resident 1920x1080 and
1280x720 frames, packed RGB and planar I420, resized to 280x192 under stretch, letterbox and crop (frame_grabber.fit_geometry),
timed with HIP events around the call: one warm-up, then --reps repetitions, the median reported with the fastest and slowest.

    python tools/fit_probe.py [--frames 512] [--reps 9] [--plain-only]

The yardstick is a library of the PARENT commit on the same frames in the same session, never the new code: run the probe with
IIV_LIB naming that library and --plain-only (it has the plain entry points alone), alternated with runs of this build, and read
the session's run-to-run spread off the repeated plain lines (profiles/fit_probe.txt).  Lines:
    plain      iiv_resize_frames / iiv_resize_frames_yuv420 (either library)
    stretch    the whole frame over the whole destination through iiv_resize_frames_fit / iiv_resize_frames_yuv420_fit
    letterbox  the whole frame into the centred rectangle, the fill colour around it
    crop       the centred 4:3 box over the whole destination"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = [(1080, 1920), (720, 1280)]
SIZE = (192, 280)


def timed(torch, call, reps):
    call()                                                    # warm: tables, code objects, the scratch pool
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--plain-only", action="store_true", help="the plain entry points alone: all a parent library has")
    a = ap.parse_args()
    import torch
    import _iiv_native as native
    from resize_probe import synth
    print("fit probe -> 280x192 on %s, library %s, build %s, %d frames, 1 warm-up + %d repetitions" % (
        torch.cuda.get_device_name(0), os.path.relpath(native.LIB_PATH, ROOT), native.build_id(), a.frames, a.reps), flush=True)
    out = torch.empty((a.frames,) + SIZE + (3,), dtype=torch.uint8, device="cuda")
    for (h, w) in SIZES:
        rgb = synth(torch, a.frames, h, w)
        y = rgb[..., 1].contiguous()
        u = rgb[:, ::2, ::2, 2].contiguous()
        v = rgb[:, ::2, ::2, 0].contiguous()
        modes = [("plain", {})]
        if not a.plain_only:
            import frame_grabber
            for fit in frame_grabber.FITS:
                box, rect = frame_grabber.fit_geometry(h, w, SIZE[0], SIZE[1], fit)
                modes.append((fit, dict(box=box, rect=rect, fill=(16, 32, 64))))
        for kind, call in (("rgb", lambda kw: native.resize_frames(rgb, SIZE, out=out, **kw)),
                           ("i420", lambda kw: native.resize_frames_yuv420(y, u, v, SIZE, out=out, **kw))):
            for name, kw in modes:
                med, lo, hi = timed(torch, lambda: call(kw), a.reps)
                print("%4dx%-4d %-4s %-9s %.3f ms (fastest %.3f, slowest %.3f) = %.0f frames/s" % (
                    w, h, kind, name, med, lo, hi, a.frames / med * 1e3), flush=True)
        del rgb, y, u, v


if __name__ == "__main__":
    main()
