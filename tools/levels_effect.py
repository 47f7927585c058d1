"""What --levels auto does to an encoded clip (profiles/levels_effect.txt): tools/transcode_clip.py's test card squeezed
into LO..HI, encoded Movie-paced with and without Levels(auto=True), in DHGR colour and on a monochrome monitor (Palette.MONO), and
after each source frame's opcodes the screen measured against the UNSQUEEZED card (StreamBatch.screens_error, per unit of sixteen
dots) -- the picture the viewer was meant to see, not the squeezed one the ingest was given.

    python tools/levels_effect.py [--frames 12] [--range 64,160] [--dither 32] [--seed 1]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--range", default="64,160")
    ap.add_argument("--dither", default="32")
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

    lo, hi = (int(v) for v in a.range.split(","))
    mode = native.DHGR
    dither = int(a.dither) if a.dither.isdigit() else a.dither
    print("levels effect on %s, build %s: %d frames of the test card squeezed into %d..%d, DHGR, dither %s, seed %d" % (
        torch.cuda.get_device_name(0), native.build_id(), a.frames, lo, hi, a.dither, a.seed))
    for pal_id in (palette.Palette.NTSC, palette.Palette.MONO):
        width = native.MONO_SIZE[mode][1] if pal_id == palette.Palette.MONO else 280
        clean = transcode_clip.test_card(a.frames, width)
        squeezed = transcode_clip.squeeze(clean, lo, hi)
        ref = torch.from_numpy(clean).cuda()
        dm = palette.diff_matrix(pal_id)
        table, store = native.build_table(mode, dm, True), native.build_store_table(mode, dm)
        db, report = {}, None
        for name, levels in (("plain", None), ("auto", frame_grabber.Levels(auto=True))):
            grab = frame_grabber.ArrayFrameGrabber(squeezed, video_mode.VideoMode.DHGR, pal_id, dither=dither, levels=levels)
            main_maps, aux_maps = grab.memory_maps()
            if levels is not None:
                report = grab.levels_report()
            batch = stream_batch.StreamBatch(mode, table, store, 1, seeds=[(a.seed, a.seed)], dm=dm, input_frame_rate=grab.input_frame_rate)
            frames_main, frames_aux = main_maps[None], aux_maps[None] if aux_maps is not None else None
            sums, n_ops = [], 0
            for i in range(a.frames):
                o, _ = batch.encode_frames(frames_main, frames_aux, 1)
                n_ops += int(o.shape[1])
                sums.append(batch.screens_error(ref[i:i + 1], pal_id))
            batch.enc.check()
            host = np.stack([t.cpu().numpy()[0] for t in sums])
            db[name] = screen.psnr(host, 2)[1]
            batch.close()
            print("%-4s %-5s: %d opcodes" % (pal_id.name, name, n_ops))
        print("%s: auto found black %s, white %s" % (pal_id.name, report["black"], report["white"]))
        print("frame   unit PSNR plain   unit PSNR auto   (dB, screen after the frame's opcodes against the unsqueezed card)")
        for i in range(a.frames):
            print("%5d   %15.3f   %14.3f" % (i, db["plain"][i], db["auto"][i]))
        print("%s mean over %d frames: unit PSNR plain %.3f dB, auto %.3f dB" % (
            pal_id.name, a.frames, float(np.mean(db["plain"])), float(np.mean(db["auto"]))))


if __name__ == "__main__":
    main()
