"""Play an .a2m file on the device: check it as written, and show or score what it puts on the screen.

    python tools/play_a2m.py clip.a2m --check
    python tools/play_a2m.py clip.a2m --every 490 --preview screens.npy
    python tools/play_a2m.py clip.a2m --every 490 --ref frames.npy --quality quality.json
    python tools/play_a2m.py clip.a2m --audio out.wav [--decim 23] [--order 3] [--gain 16384] [--clock 1020484]

The file may come from tools/transcode_clip.py, from the reference's transcoder or from an older build: the reader works
from the bytes alone (include/iivision.h section f9; csrc/iiv_a2m_read.hip).  --dbg: the player's cc65 debug file the
stream was written for; without it the placeholder addresses of tools/transcode_clip.py (a2m.OpcodeAddresses.placeholder()).
--check: print the stream's status, mode and opcode count; the exit status is non-zero unless it is OK.
--every OPS: a snapshot of screen memory after every OPS opcodes (an opcode is 73 cycles, so this is uniform in time) and
one at the end of the stream; snapshot j holds the first min((j + 1) * OPS, n_ops) opcodes.
--preview OUT.npy: the snapshots drawn through the colour model (csrc/iiv_render.hip), uint8 (snapshots, 192, 560, 3).
--ref FRAMES.npy --quality OUT.json: the snapshots measured against one reference frame each, uint8 (snapshots, 192, 280 or
560, 3), on the device (csrc/iiv_render_error.hip): the nine exact sums of squared differences and three PSNRs per snapshot,
in the layout tools/transcode_clip.py --quality writes.
--audio OUT.wav: what the stream's ticks sound like, 16-bit mono PCM: the speaker's pulses, the ACKs' two periods included, through
a CIC decimator of --order stages that keeps one sample per --decim cycles, scaled by --gain / 32768 of full scale
(csrc/iiv_speaker.hip; include/iivision.h section f13).  The rate written is --clock / --decim, rounded (audio.speaker_rate)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("stream", metavar="IN.a2m")
    ap.add_argument("--dbg", help="player/iivision.dbg (opcode entry points)")
    ap.add_argument("--every", type=int, metavar="OPS", help="opcodes between two snapshots")
    ap.add_argument("--palette", choices=["NTSC", "IIGS", "MONO"], default="NTSC")
    ap.add_argument("--preview", metavar="OUT.npy")
    ap.add_argument("--ref", metavar="FRAMES.npy")
    ap.add_argument("--quality", metavar="OUT.json")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--audio", metavar="OUT.wav")
    ap.add_argument("--decim", type=int, default=23, help="cycles per sample, 1..73")
    ap.add_argument("--order", type=int, default=3, help="CIC stages, 1..4")
    ap.add_argument("--gain", type=int, default=16384, help="0..32767")
    ap.add_argument("--clock", type=int, default=1020484, help="cycles a second of the machine")
    a = ap.parse_args()
    if bool(a.ref) != bool(a.quality):
        ap.error("--ref and --quality go together")
    if (a.preview or a.quality) and (a.every is None or a.every < 1):
        ap.error("--preview / --quality need --every OPS >= 1")
    if not (a.check or a.preview or a.quality or a.audio):
        ap.error("nothing to do: one of --check, --preview, --quality, --audio")
    if not (1 <= a.decim <= 73 and 1 <= a.order <= 4 and 0 <= a.gain <= 32767 and a.clock >= 1):
        ap.error("--decim 1..73, --order 1..4, --gain 0..32767, --clock >= 1")

    import torch
    import _iiv_native as native
    import a2m
    import audio
    import palette
    import screen

    addr = a2m.OpcodeAddresses.from_debug_file(a.dbg) if a.dbg else a2m.OpcodeAddresses.placeholder()
    data = np.fromfile(a.stream, dtype=np.uint8)
    reader = a2m.A2mReader(addr)
    status, mode, n_ops, position = (int(v) for v in reader.scan([data])[0])
    name = native.A2M_STATUS[status]
    if a.check or status != native.A2M_OK:
        print("%s: %s%s, mode %s, %d opcodes, %d bytes" % (
            a.stream, name, "" if status == native.A2M_OK else " at byte %d" % position,
            {0: "HGR", 1: "DHGR"}.get(mode, mode), n_ops, len(data)))
    if status != native.A2M_OK:
        reader.close()
        return 1
    if a.preview or a.quality:
        n = max(1, -(-n_ops // a.every))
        mem_main, mem_aux = reader.replay([data], first=a.every, every=a.every, n=n)
        rgb = palette.palette_class(palette.Palette[a.palette]).rgb_array()
        if a.preview:
            np.save(a.preview, native.render_rgb(mode, rgb, mem_main[0], mem_aux[0]).cpu().numpy())
            print("%d snapshots, every %d opcodes -> %s" % (n, a.every, a.preview))
        if a.quality:
            ref = np.load(a.ref)
            if ref.ndim != 4 or ref.shape[0] != n:
                print("--ref holds %s frames, the stream gives %d snapshots" % (ref.shape[0] if ref.ndim == 4 else "no", n), file=sys.stderr)
                reader.close()
                return 2
            sums = native.render_error(mode, rgb, mem_main[0], mem_aux[0], torch.from_numpy(np.ascontiguousarray(ref)).cuda())
            host = sums.cpu().numpy()
            db = [screen.psnr(host, level)[1] for level in range(3)]
            with open(a.quality, "w") as f:
                json.dump({"mode": {0: "HGR", 1: "DHGR"}[mode], "palette": a.palette, "ref_width": int(ref.shape[2]), "every": a.every,
                           "levels": ["dot", "quad", "unit"], "channels": ["R", "G", "B"],
                           "frames": [{"frame": i, "opcodes": min((i + 1) * a.every, n_ops), "sums": [[int(v) for v in row] for row in host[i]],
                                       "psnr_db": [float(db[level][i]) for level in range(3)]} for i in range(n)]}, f, indent=1)
            print("screen against reference, mean PSNR over %d snapshots: dot %.2f dB, quad %.2f dB, unit %.2f dB -> %s" % (
                n, *(float(np.mean(d)) for d in db), a.quality))
    if a.audio:
        pcm = reader.speaker_pcm([data], a.decim, a.order, a.gain)[0].cpu().numpy()
        rate = audio.speaker_rate(a.decim, a.clock)
        audio.write_wav(a.audio, pcm, rate)
        print("%d samples at %d Hz (%.2f s) -> %s" % (len(pcm), rate, len(pcm) / rate, a.audio))
    reader.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
