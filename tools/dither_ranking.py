"""Worked example of the screen-error measurement (include/iivision.h "f8: screen error"): the synthetic test
card of tools/transcode_clip.py (or, with `pictures`, picture-like frames: smooth colour fields with edges) through the colour
ingest with no dither, ordered dither 32 and error diffusion, and through the direct ingest at amplitudes 0 and
32, each screen measured against the card on the device at the three levels -- per dot, per quad of four dots, per unit of sixteen --
and the three conversions ranked by each level.  What is measured is the ingest's own memory maps (what the screen shows
once an encoder has converged on the frame).
Direct 0 is first per dot whatever the frames: no memory map has a smaller per-dot error.
    python tools/dither_ranking.py [frames] [DHGR|HGR] [card|pictures]"""
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
kind = sys.argv[3] if len(sys.argv) > 3 else "card"


def pictures(n, seed=11):
    """(n, 192, 280, 3): a coarse random colour field enlarged smoothly, a few hard-edged rectangles on it, a little noise"""
    rng = np.random.default_rng(seed)
    coarse = torch.from_numpy(rng.integers(0, 256, (n, 3, 7, 9)).astype(np.float32))
    out = torch.nn.functional.interpolate(coarse, size=(192, 280), mode="bicubic", align_corners=False).permute(0, 2, 3, 1).numpy()
    for f in range(n):
        for _ in range(4):
            y, x = int(rng.integers(0, 150)), int(rng.integers(0, 230))
            out[f, y:y + int(rng.integers(10, 42)), x:x + int(rng.integers(10, 50))] = rng.integers(0, 256, 3)
    return np.clip(out + rng.normal(0, 3, out.shape), 0, 255).astype(np.uint8)


card = torch.from_numpy(transcode_clip.test_card(n) if kind == "card" else pictures(n)).cuda()
names = {0: "no dither", 32: "ordered dither 32", native.DITHER_DIFFUSION: 'dither="diffusion"', "direct 0": "direct 0", "direct 32": "direct 32"}
rows = {}
for dither, name in names.items():
    if isinstance(dither, str):
        main, aux = native.frames_to_memory_maps_direct(mode, pal, card, int(dither.split()[1]))
    else:
        main, aux = native.frames_to_memory_maps(mode, pal, card, dither)
    sums = screen.render_error(main, aux, mode, pal, card).cpu().numpy()
    total = sums.astype(object).sum(axis=0)                                          # over the frames: exact Python integers
    rows[name] = [float(screen.psnr(np.array(total.tolist(), dtype=np.float64) / n, level)[1]) for level in range(3)]
print("%s, NTSC palette, %d frames of %s (build %s): PSNR in dB of the mean squared error over the frames" % (
    mode_name, n, "the test card" if kind == "card" else "picture-like content", native.build_id()))
print("%-24s %10s %10s %10s" % ("", "dot", "quad", "unit"))
for name, db in rows.items():
    print("%-24s %10.2f %10.2f %10.2f" % (name, *db))
for level, what in enumerate(("dot", "quad", "unit")):
    print("ranked by %-5s %s" % (what + ":", " > ".join(sorted(rows, key=lambda k: -rows[k][level]))))
