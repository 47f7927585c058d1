"""Worked example of the screen-error measurement (include/iivision.h "f8: screen error"): the synthetic test
card of tools/transcode_clip.py through the colour ingest with no dither, ordered dither 32 and error diffusion, each
screen measured against the card on the device at the three levels -- per dot, per quad of four dots, per unit of sixteen --
and the three conversions ranked by each level.  What is measured is the ingest's own memory maps (what the screen shows
once an encoder has converged on the frame).
    python tools/dither_ranking.py [frames] [DHGR|HGR]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ii-vision_amd", "transcoder"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np, torch
import _iiv_native as native, palette, screen
import transcode_clip

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8
mode_name = sys.argv[2] if len(sys.argv) > 2 else "DHGR"
mode = native.DHGR if mode_name == "DHGR" else native.HGR
pal = palette.NTSCPalette.rgb_array()
card = torch.from_numpy(transcode_clip.test_card(n)).cuda()
names = {0: "no dither", 32: "ordered dither 32", native.DITHER_DIFFUSION: 'dither="diffusion"'}
rows = {}
for dither, name in names.items():
    main, aux = native.frames_to_memory_maps(mode, pal, card, dither)
    sums = screen.render_error(main, aux, mode, pal, card).cpu().numpy()
    total = sums.astype(object).sum(axis=0)                                          # over the frames: exact Python integers
    rows[name] = [float(screen.psnr(np.array(total.tolist(), dtype=np.float64) / n, level)[1]) for level in range(3)]
print("%s, NTSC palette, %d frames of the test card (build %s): PSNR in dB of the mean squared error over the frames" % (
    mode_name, n, native.build_id()))
print("%-22s %10s %10s %10s" % ("", "dot", "quad", "unit"))
for name, db in rows.items():
    print("%-22s %10.2f %10.2f %10.2f" % (name, *db))
for level, what in enumerate(("dot", "quad", "unit")):
    print("ranked by %-5s %s" % (what + ":", " > ".join(sorted(rows, key=lambda k: -rows[k][level]))))
