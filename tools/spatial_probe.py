"""The spatial filter's rate on the device (csrc/iiv_filter.hip, include/iivision.h f16) at 280x192: one clip of --long frames, and
--clips clips of --frames frames, each a picture under noise of -4..4, one iiv_filter_frames call timed with HIP events: one
warm-up, then --reps repetitions, the median reported with the fastest and slowest; under the binomial taps with a denoise-and-sharpen
gain, and under the identity taps with a zero gain (the same instructions on other numbers).

    python tools/spatial_probe.py [--long 1000] [--clips 1024] [--frames 64] [--reps 5]

Bytes are counted from the shapes: the kernel reads every byte of the clip once, plus its halo rows, and writes every byte once; the
halo is not counted.  The yardstick of the batch is the copy rate tools/hbm_stream reports in the same session (run it beside this;
profiles/spatial_probe.txt); the aim is half of it.  Beside the single clip stands the temporal hold of the same frames."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W = 192, 280


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--long", type=int, default=1000)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import _iiv_native as native
    import frame_grabber
    from temporal_probe import timed
    print("spatial probe on %s, build %s: %dx%d, 1 warm-up + %d repetitions" % (
        torch.cuda.get_device_name(0), native.build_id(), W, H, a.reps), flush=True)
    tables = (("binomial taps, denoise (4, 12) + sharpen (384, 16)", frame_grabber.BINOMIAL_TAPS,
               frame_grabber.filter_gain(denoise=(4, 12), sharpen=(384, 16))),
              ("identity taps, zero gain", frame_grabber.filter_taps(0), frame_grabber.filter_gain()))

    def clip(c, n):
        base = torch.randint(8, 248, (c, 1, H, W, 3), dtype=torch.uint8, device="cuda")
        return base + torch.randint(0, 9, (c, n, H, W, 3), dtype=torch.uint8, device="cuda") - 4

    for c, n in ((1, a.long), (a.clips, a.frames)):
        src = clip(c, n)
        out = torch.empty_like(src)
        moved = 2 * src.numel()
        for name, taps, gain in tables:
            med, lo_t, hi_t = timed(torch, lambda: native.filter_frames(src, taps, taps, gain, out=out), a.reps)
            print("%5d clips x %4d frames, %s: %8.3f ms (fastest %.3f, slowest %.3f): %7.1f GB/s read + written, %.0f frames/s" % (
                c, n, name, med, lo_t, hi_t, moved / med / 1e6, c * n / med * 1e3), flush=True)
        if c == 1:
            med, lo_t, hi_t = timed(torch, lambda: native.temporal_hold(src, 6, 6, out=out), a.reps)
            print("    the temporal hold (6, 6), counts off, of the same %d frames: %8.3f ms (fastest %.3f, slowest %.3f)" % (n, med, lo_t, hi_t), flush=True)
        del src, out


if __name__ == "__main__":
    main()
