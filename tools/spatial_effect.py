"""What the spatial filter does to an encoded clip (profiles/spatial_effect.txt): tools/transcode_clip.py's test card
under uniform noise of -A..A, encoded Movie-paced with the filter's denoise, its sharpen, the temporal hold, combinations of them, and
none; after each source frame's opcodes the screen is measured against the CLEAN card (StreamBatch.screens_error, per unit of
sixteen dots) -- the picture the viewer was meant to see, not the noisy one the ingest was given.  Per variant: the opcodes, the
memory-map bytes that differ from the frame before, and the unit PSNR, each a mean over frames 1..n - 1.

    python tools/spatial_effect.py [--frames 30] [--noise 3] [--denoise 4,12] [--sharpen 256,16] [--temporal 6,6] [--dither 32]
                                   [--mode DHGR] [--seed 1]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--noise", type=int, default=3)
    ap.add_argument("--denoise", default="4,12")
    ap.add_argument("--sharpen", default="256,16")
    ap.add_argument("--temporal", default="6,6")
    ap.add_argument("--dither", default="32")
    ap.add_argument("--mode", choices=["DHGR", "HGR"], default="DHGR")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import torch
    import _iiv_native as native
    import frame_grabber
    import palette
    import screen
    import stream_batch
    import transcode_clip
    import video_mode

    denoise, sharpen, pair = (tuple(int(v) for v in s.split(",")) for s in (a.denoise, a.sharpen, a.temporal))
    mode = native.DHGR if a.mode == "DHGR" else native.HGR
    pal_id = palette.Palette.NTSC
    clean = transcode_clip.test_card(a.frames)
    noisy = transcode_clip.add_noise(clean, a.noise, a.seed)
    ref = torch.from_numpy(clean).cuda()
    dm = palette.diff_matrix(pal_id)
    table, store = native.build_table(mode, dm, True), native.build_store_table(mode, dm)
    dither = int(a.dither) if a.dither.isdigit() else a.dither
    print("spatial effect on %s, build %s: %d frames of the test card, noise -%d..%d, %s, dither %s, seed %d; binomial taps, denoise %s, "
          "sharpen %s, temporal %s" % (torch.cuda.get_device_name(0), native.build_id(), a.frames, a.noise, a.noise, a.mode, a.dither, a.seed,
                                       denoise, sharpen, pair))
    S = frame_grabber.Spatial
    variants = (("none", {}),
                ("denoise", dict(spatial=S(denoise=denoise))),
                ("sharpen", dict(spatial=S(sharpen=sharpen))),
                ("denoise + sharpen", dict(spatial=S(denoise=denoise, sharpen=(sharpen[0], max(sharpen[1], denoise[1]))))),
                ("temporal", dict(temporal=pair)),
                ("denoise + temporal", dict(spatial=S(denoise=denoise), temporal=pair)),
                ("denoise + sharpen + temporal", dict(spatial=S(denoise=denoise, sharpen=(sharpen[0], max(sharpen[1], denoise[1]))), temporal=pair)))
    print("%-30s %9s  %28s  %16s  %22s" % ("variant", "opcodes", "map bytes changed per frame", "unit PSNR (dB)", "ingest PSNR vs clean (dB)"))
    for name, kw in variants:
        grab = frame_grabber.ArrayFrameGrabber(noisy, video_mode.VideoMode[a.mode], pal_id, dither=dither, **kw)
        main_maps, aux_maps = grab.memory_maps()
        seen = grab.ingest_frames().cpu().numpy().astype(np.float64)
        mse = ((seen - clean) ** 2).mean()
        batch = stream_batch.StreamBatch(mode, table, store, 1, seeds=[(a.seed, a.seed)], dm=dm, input_frame_rate=grab.input_frame_rate)
        frames_main, frames_aux = main_maps[None], aux_maps[None] if aux_maps is not None else None
        sums, n_ops = [], 0
        for i in range(a.frames):
            o, _ = batch.encode_frames(frames_main, frames_aux, 1)
            n_ops += int(o.shape[1])
            sums.append(batch.screens_error(ref[i:i + 1], pal_id))
        batch.enc.check()
        host = np.stack([t.cpu().numpy()[0] for t in sums])
        db = screen.psnr(host, 2)[1]
        batch.close()
        changed = [int((main_maps[i] != main_maps[i - 1]).sum() + ((aux_maps[i] != aux_maps[i - 1]).sum() if aux_maps is not None else 0))
                   for i in range(1, a.frames)]
        print("%-30s %9d  %17.0f of %7d  %16.3f  %22.3f" % (name, n_ops, float(np.mean(changed)), 8192 * (2 if aux_maps is not None else 1),
                                                          float(np.mean(db[1:])), 10 * np.log10(255.0 ** 2 / mse) if mse else float("inf")))


if __name__ == "__main__":
    main()
