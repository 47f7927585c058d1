"""The geometries that the f12 tests share (tests/test_fit_host.py, tests/test_gpu_fit.py, tests/golden/make_fit_golden.py):
the smallest shapes at which the boxed resize can still go wrong, each (name, h, w, box, (H, W), rect).  Sources are seeded
uint8 noise, so a filter that is clamped at the box's edge instead of reading the pixels beside it shows."""
import numpy as np

FILL = (17, 130, 241)   # three different bytes


def _cases():
    c = []
    # column windows: the first staged column cmin = x0 - 3 here (the box is enlarged, so the support is 3 source pixels), in
    # each residue of (3 cmin) mod 4; the rectangle's rx and rw in each residue too
    for k in range(4):
        c.append(("cols13x11_%d" % k, 13, 11, (3 + k, 0, 8 + k, 13), (16, 20), (k, 1, 10, 14)))
        c.append(("cols37x53_%d" % k, 37, 53, (12 + k, 5.5, 40 + k, 30.25), (24, 40), (4 + k, 2, 29 + k, 17)))
    # the four image edges, interior boxes with odd and even offsets, less than one pixel, the identity
    c += [
        ("edge_left", 37, 53, (0, 3, 20.5, 30), (24, 40), (0, 3, 10, 10)),          # rect flush left
        ("edge_right", 37, 53, (30.2, 3, 53, 30), (24, 40), (30, 3, 10, 10)),       # flush right
        ("edge_top", 37, 53, (5, 0, 40, 11.7), (24, 40), (5, 0, 10, 10)),           # flush top
        ("edge_bottom", 37, 53, (5, 20.3, 40, 37), (24, 40), (5, 14, 10, 10)),      # flush bottom
        ("odd_odd", 37, 53, (7, 9, 41, 33), (24, 40), (0, 0, 40, 24)),              # the whole destination
        ("even_even", 36, 52, (8, 10, 42, 34), (24, 40), (2, 1, 35, 21)),
        ("odd_even", 37, 53, (7, 10, 47.5, 34), (24, 40), (3, 3, 13, 7)),
        ("even_odd", 36, 52, (8, 9, 50, 31.5), (24, 40), (1, 2, 38, 19)),
        ("sub_pixel", 37, 53, (20.25, 10.5, 20.75, 30.5), (24, 40), (6, 2, 5, 20)),
        ("rect_1x1", 37, 53, (3.5, 2.5, 50, 35), (24, 40), (5, 5, 1, 1)),
        ("identity", 37, 53, (10, 8, 30, 24), (24, 40), (3, 2, 20, 16)),
        ("float32_box", 37, 53, (0.1, 0.3, 52.7, 36.9), (24, 40), (1, 1, 37, 22)),   # neither end is a float32
        # pass order and path: vertical first (h > 100 w), and no horizontal pass at all (both unfused for 4:2:0 planes)
        ("tall", 301, 2, (0.5, 20.25, 2, 280.5), (24, 40), (3, 1, 9, 20)),
        ("vertical_only", 37, 53, (0, 4.5, 53, 30), (24, 60), (3, 2, 53, 17)),
        ("horizontal_only", 17, 53, (4.5, 0, 50, 17), (24, 40), (3, 2, 30, 17)),
        # sizes: a 560-wide mono target, and a staged window wider than 4096 pixels (one row a workgroup)
        ("mono560", 37, 53, (1.5, 2.5, 50.5, 33), (8, 560), (10, 1, 537, 6)),
        ("wide", 3, 4200, (10.5, 0, 4190.25, 3), (4, 40), (1, 1, 37, 2)),
    ]
    return c


CASES = _cases()
NAMES = [c[0] for c in CASES]
# one of each kind, recorded from Pillow in tests/golden/g12_fit.npz
GOLDEN = ["cols13x11_1", "cols37x53_2", "edge_left", "edge_right", "edge_top", "edge_bottom", "odd_odd", "even_even", "sub_pixel",
          "rect_1x1", "identity", "float32_box", "tall", "vertical_only", "horizontal_only", "mono560", "wide"]


def case(name):
    return CASES[NAMES.index(name)]


def source(name):
    """the case's seeded noise frame, uint8 (h, w, 3)"""
    _, h, w = case(name)[:3]
    return np.random.RandomState(1000 + NAMES.index(name)).randint(0, 256, (h, w, 3)).astype(np.uint8)


def random_geometry(rng, h, w, H, W):
    """a seeded random (box, rect): fractional and whole-pixel boxes, boxes spanning an axis"""
    kind = rng.randint(0, 4)
    x0, x1 = sorted(rng.uniform(0, w, 2))
    y0, y1 = sorted(rng.uniform(0, h, 2))
    if kind == 1:
        x0, x1, y0, y1 = np.floor(x0), np.ceil(x1), np.floor(y0), np.ceil(y1)
    if kind == 2:
        x0, x1 = 0, w
    if kind == 3:
        y0, y1 = 0, h
    if np.float32(x1) <= np.float32(x0):
        x0, x1 = 0, w
    if np.float32(y1) <= np.float32(y0):
        y0, y1 = 0, h
    rw, rh = int(rng.randint(1, W + 1)), int(rng.randint(1, H + 1))
    rect = (int(rng.randint(0, W - rw + 1)), int(rng.randint(0, H - rh + 1)), rw, rh)
    return tuple(float(np.float32(v)) for v in (x0, y0, x1, y1)), rect
