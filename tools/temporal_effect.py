"""What the temporal hold does to an encoded clip (profiles/temporal_effect.txt): tools/transcode_clip.py's test card
under uniform noise of -A..A, encoded Movie-paced with and without the hold, and after each source frame's opcodes the screen
measured against the CLEAN card (StreamBatch.screens_error, per unit of sixteen dots) -- the picture the viewer was meant to see,
not the noisy one the ingest was given.  Per frame: the share of pixels held, and the PSNR of both runs.

    python tools/temporal_effect.py [--frames 30] [--noise 3] [--temporal 6,6] [--dither 32] [--mode DHGR] [--seed 1]"""
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

    pair = tuple(int(v) for v in a.temporal.split(","))
    mode = native.DHGR if a.mode == "DHGR" else native.HGR
    pal_id = palette.Palette.NTSC
    clean = transcode_clip.test_card(a.frames)
    noisy = transcode_clip.add_noise(clean, a.noise, a.seed)
    ref = torch.from_numpy(clean).cuda()
    dm = palette.diff_matrix(pal_id)
    table, store = native.build_table(mode, dm, True), native.build_store_table(mode, dm)
    dither = int(a.dither) if a.dither.isdigit() else a.dither
    print("temporal effect on %s, build %s: %d frames of the test card, noise -%d..%d, %s, dither %s, seed %d" % (
        torch.cuda.get_device_name(0), native.build_id(), a.frames, a.noise, a.noise, a.mode, a.dither, a.seed))
    db, ops, counts = {}, {}, None
    for name, temporal in (("plain", None), ("hold", pair)):
        grab = frame_grabber.ArrayFrameGrabber(noisy, video_mode.VideoMode[a.mode], pal_id, dither=dither, temporal=temporal)
        main_maps, aux_maps = grab.memory_maps()
        if temporal is not None:
            counts = grab.temporal_counts()
        batch = stream_batch.StreamBatch(mode, table, store, 1, seeds=[(a.seed, a.seed)], dm=dm, input_frame_rate=grab.input_frame_rate)
        frames_main, frames_aux = main_maps[None], aux_maps[None] if aux_maps is not None else None
        sums, n_ops = [], 0
        for i in range(a.frames):
            o, _ = batch.encode_frames(frames_main, frames_aux, 1)
            n_ops += int(o.shape[1])
            sums.append(batch.screens_error(ref[i:i + 1], pal_id))
        batch.enc.check()
        host = np.stack([t.cpu().numpy()[0] for t in sums])
        db[name], ops[name] = screen.psnr(host, 2)[1], n_ops
        batch.close()
        changed = [int((main_maps[i] != main_maps[i - 1]).sum() + ((aux_maps[i] != aux_maps[i - 1]).sum() if aux_maps is not None else 0))
                   for i in range(1, a.frames)]
        print("%-5s: %d opcodes; memory-map bytes that differ from the frame before, mean over frames 1..%d: %.0f of %d" % (
            name, n_ops, a.frames - 1, float(np.mean(changed)), 8192 * (2 if aux_maps is not None else 1)))
    print("frame  held %  blended %  passed %   unit PSNR plain   unit PSNR hold (dB, screen after the frame's opcodes against the clean card)")
    for i in range(a.frames):
        share = 100.0 * counts[i] / counts[i].sum()
        print("%5d  %6.2f  %9.2f  %8.2f   %15.3f   %14.3f" % (i, share[0], share[1], share[2], db["plain"][i], db["hold"][i]))
    print("mean over frames 1..%d: held %.2f %%; unit PSNR plain %.3f dB, hold %.3f dB" % (
        a.frames - 1, float(np.mean(100.0 * counts[1:, 0] / counts[1:].sum(axis=1))), float(np.mean(db["plain"][1:])),
        float(np.mean(db["hold"][1:]))))


if __name__ == "__main__":
    main()
