"""What the spatial-filter tests share (tests/test_gpu_spatial.py, tests/test_gpu_spatial_batches.py,
tests/test_spatial_batches_host.py, tests/test_spatial_model.py): the case grid, the inputs, the constants mirrored from
csrc/iiv_clip.h and csrc/iiv_filter.hip, and the model's output of each, computed once and shared read-only.

The filter is stateless per frame and per clip, so the model of the first n frames of the first c clips is the front of the model of
the whole (CLIPS, FRAMES) block, and the blur depends on the taps alone: one blur per (H, W, tap pair) serves every gain, frame count
and clip count of the grid."""
import functools

import numpy as np

import spatial_model as M

# mirrored from csrc/iiv_clip.h (the clip stages' shared three) and csrc/iiv_filter.hip (the tile);
# tests/test_spatial_batches_host.py reads them from the text and fails if they moved
THREADS = 256               # iiv_clip.h: constexpr int kClipThreads = 256
LANE_PIXELS = 4             # iiv_clip.h: constexpr int kClipLanePixels = 4
GRID_CAP = 2048             # iiv_clip.h: constexpr int kClipGridCap = 2048: workgroups of a launch
T_H = 16                    # iiv_filter.hip: constexpr int kFilterTileH = 16: rows of a tile
T_W = 320                   # iiv_filter.hip: constexpr int kFilterTileW = 320: pixels of a tile's row
HALO = 2                    # iiv_filter.hip: constexpr int kFilterHalo = 2: rows above and below, pixels left and right

# ---- the case grid ---------------------------------------------------------------------------------------------------------------

HEIGHTS = (1, 2, 3, 4, 5, T_H - 1, T_H, T_H + 1, 2 * T_H + 3, 192)
WIDTHS = (4, 8, 12, 280, 560, T_W - 4, T_W, T_W + 4)
N_FRAMES = (1, 3)
N_CLIPS = (1, 3)
CLIPS, FRAMES = max(N_CLIPS), max(N_FRAMES)
SENTINEL = 0x5B             # tests/stream_probe.py's SENTINEL_B

IDENTITY_TAPS = (0, 0, 256, 0, 0)
BINOMIAL_TAPS = (16, 64, 96, 64, 16)
ASYMMETRIC_TAPS = (10, 20, 100, 80, 46)
TAP_PAIRS = ((IDENTITY_TAPS, IDENTITY_TAPS), (BINOMIAL_TAPS, BINOMIAL_TAPS), (ASYMMETRIC_TAPS, BINOMIAL_TAPS),
             (BINOMIAL_TAPS, ASYMMETRIC_TAPS))


def gain_table(denoise=None, sharpen=None):
    """frame_grabber.filter_gain restated in Python integers: int16 (256,)"""
    g = [0] * 256
    if denoise is not None:
        lo, hi = denoise
        g = [-256 if m <= lo else -256 + (256 * (m - lo)) // (hi - lo + 1) if m <= hi else 0 for m in range(256)]
    if sharpen is not None:
        amount, threshold = sharpen
        g = [amount if m > threshold else g[m] for m in range(256)]
    return np.array(g, np.int16)


def _frozen(a):
    a.setflags(write=False)
    return a


GAINS = {
    "zero": _frozen(np.zeros(256, np.int16)),
    "blur": _frozen(np.full(256, -256, np.int16)),
    "most": _frozen(np.full(256, 1024, np.int16)),
    "both": _frozen(gain_table(denoise=(4, 12), sharpen=(384, 16))),
    "random": _frozen(np.random.default_rng(1600).integers(-256, 1025, 256).astype(np.int16)),
}


def seams(size, tile):
    """the first index of every tile behind the first"""
    return list(range(tile, size, tile))


def impulse_points(H, W):
    """(y, x) of the single impulses: each corner, the middle of each edge, both sides of every tile seam, and the two pixels that
    meet diagonally where a row seam crosses a column seam; without repeats, in a fixed order"""
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
    for s in seams(H, T_H):
        pts += [(s - 1, W // 2), (s, W // 2)]
    for c in seams(W, T_W):
        pts += [(H // 2, c - 1), (H // 2, c)]
        for s in seams(H, T_H):
            pts += [(s - 1, c - 1), (s, c)]
    return list(dict.fromkeys(pts))


N_IMPULSE_FRAMES = CLIPS * FRAMES - 3


@functools.lru_cache(maxsize=None)
def block(H, W):
    """uint8 (CLIPS, FRAMES, H, W, 3).  Clip 0: uniform noise, a constant, a 0/255 checkerboard.  The six frames of clips 1 and 2: the
    impulses of impulse_points, 255 on black, dealt round the frames in turn so that neighbours land in different frames."""
    rng = np.random.default_rng(1601 + 7 * H + W)
    a = np.zeros((CLIPS * FRAMES, H, W, 3), np.uint8)
    a[0] = rng.integers(0, 256, (H, W, 3))
    a[1] = 137
    y, x = np.mgrid[0:H, 0:W]
    a[2] = (255 * ((x + y) & 1))[..., None]
    for i, (py, px) in enumerate(impulse_points(H, W)):
        a[3 + i % N_IMPULSE_FRAMES, py, px] = 255
    return _frozen(a.reshape(CLIPS, FRAMES, H, W, 3))


@functools.lru_cache(maxsize=None)
def blurred(H, W, pair):
    return _frozen(M.blur(block(H, W), *TAP_PAIRS[pair]))


def want(H, W, pair, gain):
    """the model of the whole block under TAP_PAIRS[pair] and GAINS[gain]: uint8 (CLIPS, FRAMES, H, W, 3)"""
    return M.blend(block(H, W), blurred(H, W, pair), GAINS[gain])


# ---- past the first trip of the grid-stride loop -----------------------------------------------------------------------------------

BATCH_W = 4                 # one quad a row
BATCH_HEIGHTS = (1, T_H + 1)     # one tile a frame, and two
BATCH_FRAMES = 1
BATCH_TAPS = (ASYMMETRIC_TAPS, BINOMIAL_TAPS)
BATCH_GAIN = "both"
P = 7                       # clips in the pool


def tiles(H, W):
    return -(-H // T_H) * -(-W // T_W)


def trips(n_clips, H, W=BATCH_W, n_frames=BATCH_FRAMES):
    """grid-stride trips the busiest workgroup makes"""
    return -(-n_clips * n_frames * tiles(H, W) // GRID_CAP)


def least_clips(trip, H):
    """the least clip count whose launch has a `trip`-th trip"""
    return -(-((trip - 1) * GRID_CAP + 1) // (BATCH_FRAMES * tiles(H, BATCH_W)))


def assert_trips(n, H):
    second, third = least_clips(2, H), least_clips(3, H)
    assert n in (second, third)
    assert trips(second - 1, H) == 1 and trips(second, H) == 2 and trips(third - 1, H) == 2 and trips(third, H) == 3
    # the clip a workgroup meets on a later trip is never the pool item it had on an earlier one
    per_clip = BATCH_FRAMES * tiles(H, BATCH_W)
    for k in range(1, trips(n, H)):
        assert (k * GRID_CAP) % per_clip == 0 and ((k * GRID_CAP) // per_clip) % P != 0


@functools.lru_cache(maxsize=None)
def pool(H):
    """uint8 (P, BATCH_FRAMES, H, BATCH_W, 3): a picture under noise of -8..8, so that the gain's three branches are met"""
    rng = np.random.default_rng(1671 + H)
    a = rng.integers(0, 256, (P, BATCH_FRAMES, 1, 1, 3)) + rng.integers(-8, 9, (P, BATCH_FRAMES, H, BATCH_W, 3))
    a[:, :, ::3, 1] += 60
    return _frozen(np.clip(a, 0, 255).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def pool_want(H):
    return _frozen(M.filter_frames(pool(H), BATCH_TAPS[0], BATCH_TAPS[1], GAINS[BATCH_GAIN]))
