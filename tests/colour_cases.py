"""The committed case set of the colour-difference tests: the palettes that go through iiv_cie2000_matrix and the pool of 1000
Lab pairs that goes through iiv_delta_e_cie2000, with tests/colour_model.py's values of them (computed once a session).
tests/test_colour_model.py holds the host oracle to the model on these cases and checks the conditions on the set itself;
tests/test_gpu_colour.py holds the device to the model on the same cases.

Conditions (tests/test_colour_model.py asserts them; a draw that fails one is drawn again from the same generator):
    palettes   every off-diagonal delta-E of the model is below 1e-9 (the same colour twice) or more than 1e-6 from an
               integer: int() of it goes into the tables, and no libm is 1e-6 off
    Lab pairs  each of colour_model.margins is above 1e-6 degrees, or the pair lies on that discontinuity exactly, in a way the
               model decides exactly (colour_model's docstring): |h1' - h2'| = 180 of an exact-axis or antipodal pair, h' = 0
               of a colour with b == 0.  Eleven of Sharma's 34 pairs are of that kind (rows 10, 14 and 16-24), as are the
               exact-axis pairs; every other pair of the pool keeps all its margins
"""
import functools
import math

import numpy as np

import colour_model as M
import ingest_model

SEED = 2028
POOL = 1000
COUNTS = (1, 63, 64, 65, 128, 1000)      # one workgroup of 64 short, full, one over, two, many
KNIFE, SAME, MARGIN = 1e-6, 1e-9, 1e-6
AXIS_C = (1e-300, 1e-12, 1e-6, 1.0, 50.0)


def knife_edges_kept(f):
    """the palette condition on a 16 x 16 matrix of doubles"""
    d = np.asarray(f, dtype=np.float64)[~np.eye(16, dtype=bool)]
    return bool(((d < SAME) | (np.abs(d - np.rint(d)) > KNIFE)).all())


def pair_allowed(lab1, lab2):
    """the Lab-pair condition"""
    apart, h1, h2 = M.margin_terms(lab1, lab2)
    return ((apart > MARGIN or M.exact_axis(lab1, lab2) or M.antipodal(lab1, lab2))
            and all(h is None or h > MARGIN or M.on_axis(c) for h, c in ((h1, lab1), (h2, lab2))))


@functools.lru_cache(maxsize=256)
def matrix_of(rgb_bytes):
    """48 palette bytes -> (the model's matrix rounded to doubles, its floor)"""
    f, i = M.matrix(np.frombuffer(rgb_bytes, dtype=np.uint8).reshape(16, 3))
    f = M.as_float(f)
    f.setflags(write=False)
    i.setflags(write=False)
    return f, i


def draw_palette(rng, make):
    """make(rng) until the palette keeps its distance from every integer -> (palette, draws thrown away)"""
    redraws = 0
    while True:
        pal = np.ascontiguousarray(make(rng), dtype=np.uint8).reshape(16, 3)
        if knife_edges_kept(matrix_of(pal.tobytes())[0]):
            return pal, redraws
        redraws += 1


def _dark(rng):
    """all bytes in 0..23: both sides of the sRGB linear segment's end (byte 10 | 11), everything below the Lab crossover"""
    pal = rng.integers(0, 24, (16, 3))
    pal[:6] = [(10, 10, 10), (11, 11, 11), (10, 11, 0), (0, 10, 11), (23, 23, 23), (0, 0, 0)]
    return pal


def _crossover(rng):
    """bytes 18..29: t = 216 / 24389 lies between greys 23 and 24 (L = 8), so X, Y and Z take either branch by turns"""
    pal = rng.integers(18, 30, (16, 3))
    pal[:4] = [(23, 23, 23), (24, 24, 24), (29, 18, 18), (18, 29, 24)]
    return pal


PALETTE_NAMES = ("ntsc", "iigs") + tuple(ingest_model.PALETTES) + ("drawn_0", "drawn_1", "drawn_2", "drawn_3", "dark", "crossover", "greys")
GREYS = (0, 1, 10, 11, 12, 23, 24, 25, 64, 127, 128, 129, 200, 253, 254, 255)


@functools.lru_cache(maxsize=None)
def palettes():
    """name -> (16, 3) uint8, in a fixed order"""
    import oracle
    out = {"ntsc": oracle.PALETTE_RGB[5], "iigs": oracle.PALETTE_RGB[0]}
    out.update(ingest_model.PALETTES)      # among them the cube's corners twice ("corners") and one colour 16 times ("all_equal")
    for k in range(4):
        out["drawn_%d" % k] = draw_palette(np.random.default_rng([SEED, k]), lambda rng: rng.integers(0, 256, (16, 3)))[0]
    out["dark"] = draw_palette(np.random.default_rng([SEED, 10]), _dark)[0]
    out["crossover"] = draw_palette(np.random.default_rng([SEED, 11]), _crossover)[0]
    out["greys"] = np.array([(g, g, g) for g in GREYS], dtype=np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def model_matrix(name):
    """-> (the model's matrix rounded to doubles, its floor)"""
    return matrix_of(np.ascontiguousarray(palettes()[name], dtype=np.uint8).tobytes())


# ---- the pool of Lab pairs --------------------------------------------------------------------------------------------

def _G(C1, C2):
    c7 = ((C1 + C2) / 2) ** 7
    return 0.5 * (1 - math.sqrt(c7 / (c7 + 25.0 ** 7)))


def from_primed(L1, C1p, h1p, L2, C2p, h2p):
    """the Lab pair whose primed chromas and hues (degrees) are the given ones, to double rounding: a' = (1 + G) a, and G hangs
    on the unprimed chromas, so a fixed point"""
    G = 0.0
    for _ in range(60):
        a1, b1 = C1p * math.cos(math.radians(h1p)) / (1 + G), C1p * math.sin(math.radians(h1p))
        a2, b2 = C2p * math.cos(math.radians(h2p)) / (1 + G), C2p * math.sin(math.radians(h2p))
        G = _G(math.hypot(a1, b1), math.hypot(a2, b2))
    return (L1, a1, b1), (L2, a2, b2)


EDGE = 1e-4                      # degrees either side of a discontinuity
EDGE_CHROMAS = (0.01, 2.5, 100.0)
EDGE_HUES = (0.3, 37.0, 123.0, 200.0, 275.0, 301.0)


def _structured():
    """[(kind, lab1, lab2)]: every pair of the pool that is not a draw"""
    from test_cie2000_published import SHARMA
    out = [("sharma", tuple(r[0:3]), tuple(r[3:6])) for r in SHARMA]
    for c in AXIS_C:
        out += [("axis", (50.0, c, 0.0), (50.0, -c, 0.0)), ("axis", (50.0, c, 0.0), (50.0, -c, -0.0)),
                ("axis", (50.0, 0.0, c), (50.0, 0.0, -c)), ("axis", (50.0, 0.0, 0.0), (50.0, c, c))]
    for lab in ((50.0, 2.5, -1.0), (0.0, 0.0, 0.0), (100.0, 0.0, 0.0), (37.5, -80.0, 93.25), (99.0, 127.0, -128.0), (1.0, -1e-3, 2e-3),
                (63.0109, -31.0961, -5.8663), (50.0, 1e-300, 1e-300)):
        out.append(("identical", lab, lab))
    out.append(("black and white", (0.0, 0.0, 0.0), (100.0, 0.0, 0.0)))
    # Sharma's rows 9-16 moved: EDGE either side of |h1' - h2'| = 180, at other hues and chromas
    for h in EDGE_HUES:
        for C in EDGE_CHROMAS:
            for side in (-EDGE, EDGE):
                out.append(("near 180",) + from_primed(50.0, C, h, 50.0, C, (h + 180.0 + side) % 360.0))
    # ... and either side of h' = 0, against a colour elsewhere
    for other in (100.0, 250.0):
        for C in EDGE_CHROMAS:
            for h in (EDGE, 360.0 - EDGE):
                out.append(("near 0",) + from_primed(50.0, C, h, 55.0, C, other))
    # the mean hue either side of 275, where the rotation term peaks: as a plain mean, and as the always-add-360 mean of two
    # hues more than 180 apart (2 and 188: a plain circular mean would be 95)
    for C in (30.0, 100.0):
        for d in (-5.0, -0.5, 0.5, 5.0):
            out.append(("mean 275",) + from_primed(50.0, C, 265.0 + d, 52.0, C + 5.0, 285.0 + d))
        for d in (-0.5, 0.5):
            out.append(("mean 275, 360 added",) + from_primed(50.0, C, 2.0 + d, 52.0, C + 5.0, 188.5 + d))
    for L1, L2 in ((30.0, 70.0), (50.0, 50.0), (0.0, 100.0), (12.5, 87.5)):
        out.append(("mean L 50", (L1, 20.0, -35.0), (L2, -12.0, 8.0)))
    pal = palettes()["drawn_0"]
    labs = [M.lab_double(row) for row in pal]
    out += [("palette", labs[i], labs[j]) for i in range(16) for j in range(16)]
    return out


@functools.lru_cache(maxsize=None)
def pool():
    """-> (kinds, lab1 (POOL, 3) float64, lab2 (POOL, 3) float64): the structured pairs, then uniform Lab over
    [0, 100] x [-128, 128]^2"""
    rows = _structured()
    rng = np.random.default_rng([SEED, 20])
    while len(rows) < POOL:
        a, b = (tuple(float(v) for v in rng.uniform((0, -128, -128), (100, 128, 128))) for _ in range(2))
        if pair_allowed(a, b):
            rows.append(("uniform", a, b))
    kinds = tuple(r[0] for r in rows)
    lab1, lab2 = (np.array([r[k] for r in rows], dtype=np.float64) for k in (1, 2))
    lab1.setflags(write=False)
    lab2.setflags(write=False)
    return kinds, lab1, lab2


@functools.lru_cache(maxsize=None)
def model_pool():
    """the model's delta-E of every pair of the pool, rounded to doubles"""
    _, lab1, lab2 = pool()
    out = np.array([float(M.delta_e(tuple(a.tolist()), tuple(b.tolist()))) for a, b in zip(lab1, lab2)])
    out.setflags(write=False)
    return out


def subset(n):
    """which n pairs of the pool a call of n pairs takes, in which order: pair k sits in another lane or workgroup from call to
    call"""
    return np.random.default_rng([SEED, 30, n]).permutation(POOL)[:n]
