"""The temporal hold's rate on the device (csrc/iiv_temporal.hip, include/iivision.h f14) at 280x192: one clip of --long frames, and
--clips clips of --frames frames, each a still picture under noise of -4..4, one iiv_temporal_hold call timed with HIP events: one
warm-up, then --reps repetitions, the median reported with the fastest and slowest; with and without the counts.

    python tools/temporal_probe.py [--long 1000] [--clips 1024] [--frames 64] [--lo 6] [--hi 6] [--reps 5]

Bytes are counted from the shapes: the kernel reads and writes every byte of the clip once.  The yardstick of the batch is the copy
rate tools/hbm_stream reports in the same session (run it beside this; profiles/temporal_probe.txt); the aim is half of it.  Beside
the single clip stands the ordered-dither ingest (iiv_frames_to_memory_maps) of the same frames: the hold must not become the
slowest front-end stage of a batch."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))

H, W = 192, 280


def timed(torch, call, reps):
    call()
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
    ap.add_argument("--long", type=int, default=1000)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--lo", type=int, default=6)
    ap.add_argument("--hi", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import _iiv_native as native
    import palette
    print("temporal probe on %s, build %s: %dx%d, (lo, hi) = (%d, %d), 1 warm-up + %d repetitions" % (
        torch.cuda.get_device_name(0), native.build_id(), W, H, a.lo, a.hi, a.reps), flush=True)

    def clip(c, n):
        base = torch.randint(8, 248, (c, 1, H, W, 3), dtype=torch.uint8, device="cuda")
        return base + torch.randint(0, 9, (c, n, H, W, 3), dtype=torch.uint8, device="cuda") - 4

    for c, n in ((1, a.long), (a.clips, a.frames)):
        src = clip(c, n)
        out = torch.empty_like(src)
        moved = 2 * src.numel()
        for with_counts in (True, False):
            state = [None]

            def call():
                state[0] = native.temporal_hold(src, a.lo, a.hi, out=out, counts=with_counts)
            med, lo_t, hi_t = timed(torch, call, a.reps)
            held = ""
            if with_counts:
                k = state[0][2].to(torch.int64).sum(dim=(0, 1)).cpu().numpy()
                held = "; held %.1f %%, blended %.1f %%, passed %.1f %% of the pixels" % tuple(100.0 * k / k.sum())
            print("%5d clips x %4d frames, counts %-3s: %8.3f ms (fastest %.3f, slowest %.3f): %7.1f GB/s read + written, %.0f frames/s%s" % (
                c, n, "on" if with_counts else "off", med, lo_t, hi_t, moved / med / 1e6, c * n / med * 1e3, held), flush=True)
        if c == 1:
            pal = palette.PALETTES[palette.Palette.NTSC].rgb_array()
            frames = src[0]
            maps = native.frames_to_memory_maps(native.DHGR, pal, frames, 32)
            med, lo_t, hi_t = timed(torch, lambda: native.frames_to_memory_maps(native.DHGR, pal, frames, 32, out=maps), a.reps)
            print("    the ordered-dither ingest (DHGR, dither 32) of the same %d frames: %8.3f ms (fastest %.3f, slowest %.3f): %.0f frames/s" % (
                n, med, lo_t, hi_t, n / med * 1e3), flush=True)
        del src, out


if __name__ == "__main__":
    main()
