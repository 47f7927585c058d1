"""The speaker preview's rate on the device (csrc/iiv_speaker.hip, include/iivision.h f13): --streams device-resident streams of
--ticks ticks each, one iiv_speaker_pcm call timed with HIP events: one warm-up, then --reps repetitions, the median reported with
the fastest and slowest.

    python tools/speaker_probe.py [--streams 4096] [--ticks 882000] [--decim 23] [--order 3] [--reps 5]

Bytes are counted from the shapes: one byte read per tick, two written per sample.  The yardstick is the write rate tools/hbm_stream
reports in the same session (run it beside this; profiles/speaker_probe.txt); the aim is half of it."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=14700 * 60)
    ap.add_argument("--decim", type=int, default=23)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--gain", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import _iiv_native as native
    m = native.speaker_sample_count(a.ticks, a.decim)
    print("speaker probe on %s, build %s: %d streams x %d ticks -> %d samples each, decim %d, order %d, 1 warm-up + %d repetitions" % (
        torch.cuda.get_device_name(0), native.build_id(), a.streams, a.ticks, m, a.decim, a.order, a.reps), flush=True)
    ticks = torch.randint(0, 32, (a.streams, a.ticks), dtype=torch.uint8, device="cuda") * 2 + 4
    out = torch.empty((a.streams, -(-m // 8) * 8), dtype=torch.int16, device="cuda")
    counts = torch.full((a.streams,), a.ticks, dtype=torch.int64, device="cuda")
    L = native.lib()

    def call():
        native.check(L.iiv_speaker_pcm(a.streams, native.dptr(ticks), a.ticks, native.dptr(counts), 1, a.decim, a.order, a.gain,
                                       native.dptr(out), int(out.shape[1]), None, native.stream_ptr()))
    call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(a.reps):
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    med = times[len(times) // 2]
    read, written = a.streams * a.ticks, a.streams * m * 2
    print("%.3f ms (fastest %.3f, slowest %.3f): %.1f GB/s written + %.1f GB/s read = %.1f GB/s; %.2f G samples/s" % (
        med, times[0], times[-1], written / med / 1e6, read / med / 1e6, (read + written) / med / 1e6, a.streams * m / med / 1e6),
        flush=True)


if __name__ == "__main__":
    main()
