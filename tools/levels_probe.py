"""The rates of the two picture-levels kernels on the device (csrc/iiv_levels.hip, include/iivision.h f15) at 280x192: --clips clips
of --frames frames and one clip of --long frames, one call of each kernel timed with HIP events: one warm-up, then --reps
repetitions, the median reported with the fastest and slowest.  The histogram is measured on noise AND on flat frames (every lane
of a wave on one bin); the ratio of the two decides whether its wave-level pre-combine stays.

    python tools/levels_probe.py [--long 1000] [--clips 1024] [--frames 64] [--reps 5]
    IIV_LIB=ab/libiiv_levels_nocombine.so python tools/levels_probe.py       # the build with -DIIV_LEVELS_NO_COMBINE

Bytes are counted from the shapes: the histogram reads every byte of the clip once (its output, 4 KiB a frame, is counted too),
apply reads and writes every byte once.  The yardsticks are the read rate and the copy rate tools/hbm_stream reports in the same
session (run it beside this; profiles/levels_probe.txt); the aim is half of each."""
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
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    import _iiv_native as native
    import frame_grabber
    print("levels probe on %s, build %s (%s): %dx%d, 1 warm-up + %d repetitions" % (
        torch.cuda.get_device_name(0), native.build_id(), os.path.basename(native.LIB_PATH), W, H, a.reps), flush=True)
    lut, m, _, _ = native.levels_tables(frame_grabber.levels_lut(16, 235, gamma=1.2), frame_grabber.saturation_matrix(320).astype(np.int64), 1)
    d_lut, d_m = torch.from_numpy(lut).cuda(), torch.from_numpy(m).cuda()
    L, pixels, fb = native.lib(), H * W, H * W * 3
    for c, n in ((a.clips, a.frames), (1, a.long)):
        noise = torch.randint(0, 256, (c, n, H, W, 3), dtype=torch.uint8, device="cuda")
        hist = torch.empty((c, n, 4, 256), dtype=torch.int32, device="cuda")
        rates = {}
        for kind in ("noise", "flat"):
            src = noise if kind == "noise" else torch.full_like(noise, 97)

            def call():
                native.check(L.iiv_levels_histogram(c, n, pixels, native.dptr(src), n * fb, fb, native.dptr(hist), native.stream_ptr()))
            med, lo_t, hi_t = timed(torch, call, a.reps)
            assert int(hist[0, 0, 3].sum()) == pixels
            moved = src.numel() + hist.numel() * 4
            rates[kind] = med
            print("histogram %5d clips x %4d frames, %-5s: %8.3f ms (fastest %.3f, slowest %.3f): %7.1f GB/s read (+ 4 KiB a frame written), %.0f frames/s" % (
                c, n, kind, med, lo_t, hi_t, moved / med / 1e6, c * n / med * 1e3), flush=True)
            if kind == "flat":
                del src
        print("    flat / noise = %.2f" % (rates["flat"] / rates["noise"]), flush=True)
        out = torch.empty_like(noise)

        def call():
            native.check(L.iiv_levels_apply(c, n, pixels, native.dptr(noise), n * fb, fb, native.dptr(out), n * fb, fb, native.dptr(d_lut), 0,
                                            native.dptr(d_m), 0, native.stream_ptr()))
        med, lo_t, hi_t = timed(torch, call, a.reps)
        print("apply     %5d clips x %4d frames       : %8.3f ms (fastest %.3f, slowest %.3f): %7.1f GB/s read + written, %.0f frames/s" % (
            c, n, med, lo_t, hi_t, 2 * noise.numel() / med / 1e6, c * n / med * 1e3), flush=True)
        del noise, out, hist


if __name__ == "__main__":
    main()
