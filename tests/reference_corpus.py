"""The reference corpus (tests/golden/g11_*.npz): what its cases are, and how a test reads them back.

g3 / g7 / g8 record the reference on uniform noise only (S-iid, S-coh).  This corpus records it on the content on which
the encoder takes its other paths: picture-like frames, where most steps are decided by the nonces (`img`, `dither`,
`flat`), and converging frames, where the work list runs dry, the re-queued bag is gone through and the generator ends
out of work and pads (`static`).  tests/golden/make_golden.py --corpus-only records it; test_reference_corpus.py holds the
oracle to it on the CPU, test_gpu_reference_corpus.py every kernel form on the device.

No device is used here and nothing of the reference is imported: the builders are numpy (and the project's own CPU
generators).  The fixture stores every case's frames, so the recordings do not depend on a numpy or torch generator
staying stable; test_reference_corpus.py compares the builders with the stored frames only as a note about the builders.

    cases()          the list of Case
    load(golden)     {tag: record} from the fixture(s), a record being the dict of a case's arrays
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HGR, DHGR = 0, 1
NTSC, IIGS = 5, 0
MAX_OPS = 8000                  # no case is longer than this
FIXTURES = ("g11_reference_corpus", "g11_hgr", "g11_dhgr")     # one file, or split by mode (whichever were written)
TIE_KINDS = ("img", "dither", "flat")                           # the kinds whose steps the nonces must decide
HOLES = (np.arange(256) & 127) >= 120


def _project_paths():
    for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "ii-vision_amd", "transcoder"), os.path.join(ROOT, "tools"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)


class Case:
    def __init__(self, tag, kind, mode, palette, seed_py, seed_np, build, schedule, exhaust=False, fourth=False):
        self.tag, self.kind, self.mode, self.palette = tag, kind, mode, palette
        self.seed_py, self.seed_np = seed_py, seed_np
        self._build, self._schedule = build, schedule
        self.exhaust, self.fourth = exhaust, fourth
        self._frames = None

    @property
    def mode_name(self):
        return "DHGR" if self.mode == DHGR else "HGR"

    def frames(self):
        """(n_frames, banks, 32, 256) uint8"""
        if self._frames is None:
            f = np.ascontiguousarray(self._build(), dtype=np.uint8)
            assert f.ndim == 4 and f.shape[1:] == (2 if self.mode == DHGR else 1, 32, 256), (self.tag, f.shape)
            self._frames = f
        return self._frames

    def schedule(self):
        """[(frame, is_aux, n_ops)], one generator each.  An exhaustion case's lengths come from the oracle (recording time)."""
        s = self._schedule(self) if callable(self._schedule) else self._schedule
        s = [tuple(int(x) for x in g) for g in s]
        assert sum(g[2] for g in s) <= MAX_OPS, (self.tag, sum(g[2] for g in s))
        return s

    def meta(self):
        return np.array([self.mode, self.palette, self.seed_py, self.seed_np, int(self.fourth), int(self.exhaust)], dtype=np.int32)


# ---- content ----------------------------------------------------------------------------------------------------------

def img_frames(mode, n_frames, seed):
    """S-img: the dithered moving bars of stream_batch.synth_frames_img, on the CPU"""
    _project_paths()
    import stream_batch
    main, aux = stream_batch.synth_frames_img(1, n_frames, mode == DHGR, seed, device="cpu")
    banks = [main[0].numpy()] + ([aux[0].numpy()] if mode == DHGR else [])
    return np.stack(banks, axis=1)


def img_parameters(seed):
    """(period, speed, slope, phase) that synth_frames_img draws for its one stream under `seed`"""
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return tuple(int(torch.randint(lo, hi, (1, 1, 1), generator=g)) for lo, hi in ((24, 120), (1, 6), (-2, 3), (0, 120)))


def static_frames(mode, n_frames, seed):
    """S-static as test_gpu_configs.py's "static4": 2 % of the bytes redrawn, every drawn frame shown four times"""
    _project_paths()
    import stream_batch
    main, aux = stream_batch.synth_frames_torch(1, n_frames, mode == DHGR, seed, coherent=True, keep=0.98, repeat=4, device="cpu")
    banks = [main[0].numpy()] + ([aux[0].numpy()] if mode == DHGR else [])
    return np.stack(banks, axis=1)


def card_rgb(n_frames):
    """tools/transcode_clip.py's moving test card, (n, 192, 280, 3) uint8 (it imports without a device)"""
    _project_paths()
    import transcode_clip
    return transcode_clip.test_card(n_frames)


def dither_frames(mode, palette, n_frames, converter):
    """the test card through "ordered" (oracle.frame_to_memory_map, amplitude 32) or "fs" (the Floyd-Steinberg of
    tests/ingest_model.py)"""
    _project_paths()
    import oracle as O
    rgb = card_rgb(n_frames)
    out = np.zeros((n_frames, 2 if mode == DHGR else 1, 32, 256), np.uint8)
    for f in range(n_frames):
        if converter == "ordered":
            main, aux = O.frame_to_memory_map(mode, O.PALETTE_RGB[palette], rgb[f], 32)
        else:
            import ingest_model
            main, aux = ingest_model.frame_to_memory_map(mode, O.PALETTE_RGB[palette], rgb[f], ingest_model.DITHER_DIFFUSION)
        out[f, 0] = main
        if mode == DHGR:
            out[f, 1] = aux
    return out


def flat_frames(mode, values, row_values, y=100):
    """frame 0: one byte value per bank; frame 1: the same with the 40 bytes of screen row y changed (per bank)"""
    _project_paths()
    import oracle as O
    page, offset = O.xy_tables()
    banks = 2 if mode == DHGR else 1
    out = np.zeros((2, banks, 32, 256), np.uint8)
    for b in range(banks):
        out[:, b] = values[b]
        out[1, b, page[y].astype(int), offset[y].astype(int)] = row_values[b]
    out[:, :, :, HOLES] = 0
    return out


# ---- schedules --------------------------------------------------------------------------------------------------------

def movie_schedule(mode_name, n_frames, ops_per_frame=490):
    """make_golden.movie_schedule (movie.py:56-150 without audio), restated here so that nothing of the recorder is imported at
    test time; make_corpus_golden asserts that the two agree"""
    sched, pos, is_aux, ticks, frame_number, cur, fi = [], 7, 0, 0, 0, None, -1
    for _ in range(n_frames * ops_per_frame - 1):
        ticks += 1
        new_frame = False
        if ticks >= float(ops_per_frame) * frame_number:
            frame_number += 1
            fi += 1
            new_frame = True
        if new_frame or cur is None or cur[1] != is_aux:
            cur = [fi, is_aux, 0]
            sched.append(cur)
        cur[2] += 1
        pos += 7
        if pos % 2048 >= 2044:
            pos += 4
            if mode_name == "DHGR":
                is_aux ^= 1
    return [tuple(s) for s in sched if s[2] > 0]


def oracle_video(case, fourth=None, seed_np=None):
    _project_paths()
    import oracle as O
    O.build()
    key = (case.mode, case.palette)
    if key not in _TABLES:
        _TABLES[key] = O.build_table(case.mode, O.cie2000_matrix(O.PALETTE_RGB[case.palette])[1], symmetric=True)
    v = O.Video(case.mode, _TABLES[key], seed_py=case.seed_py, seed_np=case.seed_np if seed_np is None else seed_np)
    v.set_fourth_offset(case.fourth if fourth is None else fourth)
    return v


_TABLES = {}


def is_padding(ops, frames, fi, is_aux):
    """rows of `ops` that are the padding opcode of a generator on (frame fi, bank is_aux): page 32, the target's first
    byte, four offsets 0 (video.py:249-251)"""
    want = np.array([32, frames[fi, is_aux][0, 0], 0, 0, 0, 0], np.uint8)
    return (np.asarray(ops) == want).all(axis=1)


def to_padding(plan, pad=24):
    """A schedule whose marked generators run until the oracle pads.  plan: [(frame, is_aux, n_ops | None)]; None = as many
    opcodes as the oracle needs to come out of work on that generator, and `pad` more.  Measured, not guessed."""
    def schedule(case):
        frames, v, out = case.frames(), oracle_video(case), []
        for fi, ia, n in plan:
            v.encode_frame(frames[fi, 0], frames[fi, 1] if case.mode == DHGR else None, ia)
            if n is None:
                ops = v.next(MAX_OPS)           # (on a throw-away copy of the state: the run below starts over)
                real = int(np.nonzero(~is_padding(ops, frames, fi, ia))[0].max()) + 1 if (~is_padding(ops, frames, fi, ia)).any() else 0
                assert real < MAX_OPS and is_padding(ops[real:], frames, fi, ia).all(), (case.tag, fi, ia, "no padding within %d" % MAX_OPS)
                n = real + pad
                # replay up to here with the chosen length
                v = oracle_video(case)
                for (f2, a2, n2) in out:
                    v.encode_frame(frames[f2, 0], frames[f2, 1] if case.mode == DHGR else None, a2)
                    v.next(n2)
                v.encode_frame(frames[fi, 0], frames[fi, 1] if case.mode == DHGR else None, ia)
                v.next(n)
            else:
                v.next(n)
            out.append((fi, ia, n))
        return out
    return schedule


# ---- the cases --------------------------------------------------------------------------------------------------------

def cases():
    c = []

    def add(tag, kind, mode, pal, seeds, build, schedule, **kw):
        c.append(Case(tag, kind, mode, pal, seeds[0], seeds[1], build, schedule, **kw))

    H, D = HGR, DHGR
    # img: Movie-paced; ragged with abandoned generators; one-opcode pulls; a bank switch that comes back to a half-finished
    # frame; run to padding and on.  Four seeds = four (period, speed, slope, phase): see img_parameters().
    add("HGR_img_movie", "img", H, NTSC, (11, 12), lambda: img_frames(H, 3, 101), movie_schedule("HGR", 3))
    add("DHGR_img_movie", "img", D, NTSC, (13, 14), lambda: img_frames(D, 3, 102), movie_schedule("DHGR", 3))
    add("HGR_img_ragged_iigs", "img", H, IIGS, (15, 16), lambda: img_frames(H, 3, 103),
        [(0, 0, 183), (1, 0, 1), (1, 0, 40), (0, 0, 292), (2, 0, 3), (2, 0, 490), (1, 0, 2), (2, 0, 200)])
    add("DHGR_img_ragged_iigs", "img", D, IIGS, (17, 18), lambda: img_frames(D, 3, 104),
        [(0, 0, 183), (0, 1, 1), (1, 1, 40), (1, 0, 292), (2, 0, 3), (2, 1, 490), (1, 0, 2), (2, 0, 200)])
    add("HGR_img_single_ops", "img", H, NTSC, (19, 20), lambda: img_frames(H, 2, 101),
        [(0, 0, 1)] * 6 + [(1, 0, 1), (0, 0, 2), (1, 0, 1), (1, 0, 3)] + [(1, 0, 1)] * 8)
    add("DHGR_img_single_ops", "img", D, NTSC, (21, 22), lambda: img_frames(D, 2, 102),
        [(0, 0, 1), (0, 0, 1), (0, 1, 1), (0, 0, 2), (0, 1, 3), (1, 1, 1), (1, 0, 1), (0, 1, 1)] + [(1, 0, 1), (1, 1, 1)] * 5)
    add("HGR_img_return", "img", H, NTSC, (23, 24), lambda: img_frames(H, 3, 104),
        [(0, 0, 400), (1, 0, 150), (0, 0, 300), (2, 0, 250), (1, 0, 300)])
    add("DHGR_img_bank_return", "img", D, NTSC, (25, 26), lambda: img_frames(D, 3, 103),
        [(0, 0, 300), (0, 1, 291), (0, 0, 291), (1, 1, 200), (0, 0, 250), (1, 1, 120), (2, 0, 150)])
    add("HGR_img_exhaust", "img", H, NTSC, (27, 28), lambda: img_frames(H, 2, 103),
        to_padding([(0, 0, None), (1, 0, 120), (1, 0, None)]), exhaust=True)
    add("DHGR_img_exhaust", "img", D, NTSC, (29, 30), lambda: img_frames(D, 2, 101),
        to_padding([(0, 0, None), (0, 1, None), (1, 1, 90), (1, 0, None), (1, 1, None)]), exhaust=True)
    # static: from the list into the bag, out of work, padding, and another generator on top.  A bank of noise takes ~5000
    # opcodes from the blank screen, so the DHGR case exhausts one bank and touches only that one.  (With the other bank still
    # blank no aux byte ever reaches distance 0: every later generator finds the whole bank to do again, ~4300 opcodes.)
    add("HGR_static_exhaust", "static", H, NTSC, (31, 32), lambda: static_frames(H, 5, 201)[[0, 3, 4]],
        to_padding([(0, 0, None), (1, 0, None), (2, 0, 60), (2, 0, None)]), exhaust=True)
    add("DHGR_static_exhaust_iigs", "static", D, IIGS, (33, 34), lambda: static_frames(D, 5, 202)[[0, 3, 4]],
        to_padding([(2, 1, 60), (1, 1, 700), (0, 1, None)]), exhaust=True)   # (a second run to padding would pass 8000 opcodes)
    # dither: the moving test card, both converters, both palettes
    add("HGR_dither_ordered", "dither", H, NTSC, (35, 36), lambda: dither_frames(H, NTSC, 3, "ordered"), movie_schedule("HGR", 3, 400))
    add("DHGR_dither_ordered_iigs", "dither", D, IIGS, (37, 38), lambda: dither_frames(D, IIGS, 3, "ordered"), movie_schedule("DHGR", 3, 400))
    add("HGR_dither_fs_iigs", "dither", H, IIGS, (39, 40), lambda: dither_frames(H, IIGS, 3, "fs"),
        [(0, 0, 500), (1, 0, 1), (1, 0, 300), (2, 0, 400)])
    add("DHGR_dither_fs", "dither", D, NTSC, (41, 42), lambda: dither_frames(D, NTSC, 3, "fs"),
        [(0, 0, 291), (0, 1, 291), (1, 0, 200), (1, 1, 1), (2, 1, 300), (2, 0, 117)])
    # flat: one byte value per bank, then one row changed -- every candidate of a step shares its delta
    add("HGR_flat", "flat", H, NTSC, (43, 44), lambda: flat_frames(H, [0x2A], [0xD5]), [(0, 0, 600), (1, 0, 200), (0, 0, 100), (1, 0, 300)])
    add("DHGR_flat", "flat", D, NTSC, (45, 46), lambda: flat_frames(D, [0x2A, 0x55], [0x7F, 0x13]),
        [(0, 0, 400), (0, 1, 400), (1, 0, 150), (1, 1, 150), (0, 0, 100)])
    add("HGR_flat_iigs", "flat", H, IIGS, (47, 48), lambda: flat_frames(H, [0xD5], [0x2A], y=37), [(0, 0, 500), (1, 0, 1), (1, 0, 400)])
    add("DHGR_flat_iigs", "flat", D, IIGS, (49, 50), lambda: flat_frames(D, [0x33, 0x4C], [0x00, 0x7F], y=191),
        [(0, 1, 350), (0, 0, 350), (1, 1, 200), (1, 0, 100)])
    # the fourth offset: one img and one static per mode, recorded a second time with the reference's exit test reading 4
    # (same frames, seeds and schedule)
    base = {k.tag: k for k in c}
    for tag in ("HGR_img_movie", "DHGR_img_movie", "HGR_static_exhaust", "DHGR_static_exhaust_iigs"):
        b = base[tag]
        k = Case(tag + "_fourth", b.kind, b.mode, b.palette, b.seed_py, b.seed_np, b.frames, (lambda case, b=b: b.schedule()), exhaust=b.exhaust, fourth=True)
        k.base = b
        c.append(k)
    return c


# ---- reading the fixture ------------------------------------------------------------------------------------------------

def load(golden):
    """{tag: {name: array}} of every recording in the fixture file(s) that exist"""
    out = {}
    for name in FIXTURES:
        if not os.path.exists(os.path.join(HERE, "golden", name + ".npz")):
            continue
        g = getattr(golden, name)
        for key in g.files:
            tag, item = key.split("/")
            out.setdefault(tag, {})[item] = g[key]
    assert out, "no g11 fixture under tests/golden"
    return out
