"""What the picture-levels tests share (tests/test_gpu_levels.py, tests/test_gpu_levels_batches.py, tests/test_levels_batches_host.py,
tests/test_levels_model.py): the case grid of the issue, the five kinds of input, the constants mirrored from csrc/iiv_clip.h and
csrc/iiv_levels.hip, the tables, and the model's output of each, computed once and shared read-only.

Histograms are per frame and the tables are applied per pixel, so the model of the first n frames of the first c clips is the
front of the model of the whole (CLIPS, FRAMES) block: one model run per (pixels, kind) serves every frame and clip count."""
import functools

import numpy as np

import levels_model as M

# mirrored from csrc/iiv_clip.h (the clip stages' shared three) and csrc/iiv_levels.hip (the frames of an apply item);
# tests/test_levels_batches_host.py reads them from the text and fails if they moved
THREADS = 256               # iiv_clip.h: constexpr int kClipThreads = 256
LANE_PIXELS = 4             # iiv_clip.h: constexpr int kClipLanePixels = 4
APPLY_FRAMES = 8            # iiv_levels.hip: constexpr int kLevelsApplyFrames = 8: frames of one apply item
GRID_CAP = 2048             # iiv_clip.h: constexpr int kClipGridCap = 2048: workgroups of a launch

# ---- the case grid ---------------------------------------------------------------------------------------------------------------

PIXELS = (4, 8, 252, 256, 260, 1028, 53760)    # one lane, two; around one wave (64 lanes = 256 pixels); around one workgroup; 280x192
N_FRAMES = (1, 2, 3)
N_CLIPS = (1, 3)
KINDS = ("noise", "flat", "two", "extremes", "ramp")
CLIPS, FRAMES = max(N_CLIPS), max(N_FRAMES)
RANGE_FRAMES = 2 * APPLY_FRAMES + 1             # apply alone: two whole ranges of frames and one frame of a third
SENTINEL = 0x5B             # tests/stream_probe.py's SENTINEL_B


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def clip(kind, pixels, frames=FRAMES):
    """uint8 (CLIPS, frames, pixels, 3)"""
    rng = np.random.default_rng(1500 + KINDS.index(kind) * 100 + PIXELS.index(pixels) + 1000 * frames)
    shape = (CLIPS, frames, pixels, 3)
    if kind == "noise":
        a = rng.integers(0, 256, shape)
    elif kind == "flat":        # one colour per frame: every lane of every wave on one bin of each channel
        a = rng.integers(0, 256, (CLIPS, frames, 1, 3)) + np.zeros(shape, np.int64)
    elif kind == "two":         # two colours per frame, alternating from pixel to pixel: lane 0's value is every other lane's
        pair = rng.integers(0, 256, (CLIPS, frames, 2, 3))
        a = pair[:, :, np.arange(pixels) % 2]
    elif kind == "extremes":    # channels 0 or 255 only, whole pixels black or white in the first frame: Y reaches 0 and 255
        a = 255 * rng.integers(0, 2, shape)
        a[:, 0] = a[:, 0, :, :1]
    else:                       # a ramp along the pixels, the three channels at different offsets and slopes
        a = (np.arange(pixels)[None, None, :, None] * np.array([1, 2, 3]) + rng.integers(0, 256, (CLIPS, frames, 1, 3))) % 256
    return _frozen(a.astype(np.uint8))


@functools.lru_cache(maxsize=None)
def want_hist(kind, pixels):
    """uint32 (CLIPS, FRAMES, 4, 256)"""
    return _frozen(M.histogram(clip(kind, pixels)))


# ---- tables ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tables(name, c=CLIPS):
    """(lut uint8 (c, 3, 256), matrix int64 (c, 3, 3)): one pair per clip"""
    rng = np.random.default_rng(1550 + sum(name.encode()))
    ident = np.broadcast_to(M.IDENTITY_LUT, (c, 3, 256)).copy()
    if name == "identity":
        lut, m = ident, np.broadcast_to(M.IDENTITY_MATRIX, (c, 3, 3)).copy()
    elif name == "random":      # random tables, matrices over the whole Q8 range
        lut, m = rng.integers(0, 256, (c, 3, 256)).astype(np.uint8), rng.integers(-2048, 2048, (c, 3, 3))
    elif name == "small":       # random tables, matrices near the identity: few results clamp
        lut, m = rng.integers(0, 256, (c, 3, 256)).astype(np.uint8), M.IDENTITY_MATRIX + rng.integers(-96, 97, (c, 3, 3))
    elif name == "max":         # every entry +2047: anything but black clamps at 255
        lut, m = ident, np.full((c, 3, 3), 2047)
    elif name == "min":         # every entry -2048: anything but black clamps at 0, black stays (128 >> 8 = 0)
        lut, m = ident, np.full((c, 3, 3), -2048)
    elif name.startswith("sat"):
        lut, m = ident, np.broadcast_to(M.saturation_matrix(int(name[3:])), (c, 3, 3)).copy()
    else:
        raise KeyError(name)
    return _frozen(lut), _frozen(m.astype(np.int64))


TABLES = ("identity", "random", "small", "max", "min", "sat0", "sat256", "sat1024")


@functools.lru_cache(maxsize=None)
def want_apply(kind, pixels, name):
    """uint8 (CLIPS, FRAMES, pixels, 3): clip k through pair k of tables(name)"""
    lut, m = tables(name)
    return _frozen(M.apply_clips(clip(kind, pixels), lut, m))


def device_tables(torch, lut, m):
    """the pair on the device as the C ABI takes it: (uint8 (c, 3, 256), int16 (c, 10) -- rows of 18 bytes padded to 20)"""
    padded = np.zeros((m.shape[0], 10), np.int16)
    padded[:, :9] = m.reshape(-1, 9)
    return torch.from_numpy(np.array(lut)).cuda(), torch.from_numpy(padded).cuda()     # (a copy: the shared tables are read-only)


# ---- past the first trip of the grid-stride loops ----------------------------------------------------------------------------------

BATCH_PIXELS = 8            # two lanes: the histogram has one work item a frame, apply one a clip and range of APPLY_FRAMES frames
BATCH_FRAMES = 1            # one frame a clip: both kernels then have one work item a clip
P = 7                       # clips in the pool
N_SECOND, N_THIRD = GRID_CAP + 1, 2 * GRID_CAP + 1     # the smallest item counts with a second and with a third trip


def hist_items(n_clips, n_frames):
    return n_clips * n_frames


def apply_items(n_clips, n_frames, pixels=BATCH_PIXELS):
    return n_clips * -(-(pixels // LANE_PIXELS) // THREADS) * -(-n_frames // APPLY_FRAMES)


def trips(items):
    """grid-stride trips the busiest workgroup makes"""
    return -(-items // GRID_CAP)


def assert_trips(n):
    assert n in (N_SECOND, N_THIRD)
    for items in (hist_items, apply_items):
        assert items(n, BATCH_FRAMES) == n                      # one item a clip: no fewer clips (of any frame count) reach the trip
        assert trips(items(N_SECOND - 1, BATCH_FRAMES)) == 1 and trips(items(N_SECOND, BATCH_FRAMES)) == 2
        assert trips(items(N_THIRD - 1, BATCH_FRAMES)) == 2 and trips(items(N_THIRD, BATCH_FRAMES)) == 3
    # the clip a workgroup meets on a later trip is never the pool item it had on an earlier one
    for k in range(1, trips(n)):
        assert (k * GRID_CAP) % P != 0


@functools.lru_cache(maxsize=None)
def pool():
    """uint8 (P, BATCH_FRAMES, BATCH_PIXELS, 3) noise, with the tables of each pool clip"""
    rng = np.random.default_rng(1571)
    return _frozen(rng.integers(0, 256, (P, BATCH_FRAMES, BATCH_PIXELS, 3)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def pool_want():
    """(hist uint32 (P, BATCH_FRAMES, 4, 256), out uint8 like pool(), lut (P, 3, 256), matrix (P, 3, 3))"""
    lut, m = tables("small", P)
    return _frozen(M.histogram(pool())), _frozen(M.apply_clips(pool(), lut, m)), lut, m
