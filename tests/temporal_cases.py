"""What the temporal-hold tests share (tests/test_gpu_temporal.py, tests/test_gpu_temporal_batches.py,
tests/test_temporal_batches_host.py, tests/test_temporal_model.py, tests/test_gpu_temporal_grabber.py): the case grid of the issue,
the four kinds of input, the constants mirrored from csrc/iiv_clip.h and csrc/iiv_temporal.hip, the full-hold clip, and the model's
output of each, computed once and shared read-only.

The hold is causal and per pixel and per clip, so the model of the first n frames of the first c clips is the front of the model of
the whole (CLIPS, FRAMES) block: one model run per (pixels, kind, pair) serves every frame count and clip count of the grid."""
import functools

import numpy as np

import temporal_model as M

# mirrored from csrc/iiv_clip.h (the clip stages' shared three) and csrc/iiv_temporal.hip (the ring);
# tests/test_temporal_batches_host.py reads them from the text and fails if they moved
THREADS = 256               # iiv_clip.h: constexpr int kClipThreads = 256
LANE_PIXELS = 4             # iiv_clip.h: constexpr int kClipLanePixels = 4
RING = 8                    # iiv_temporal.hip: constexpr int kTemporalRing = 8: source frames in flight ahead of the one computed
GRID_CAP = 2048             # iiv_clip.h: constexpr int kClipGridCap = 2048: workgroups of a launch

# ---- the case grid ---------------------------------------------------------------------------------------------------------------

PIXELS = (4, 8, 252, 256, 260, 1028, 53760)    # one lane, two; around one wave (64 lanes = 256 pixels); around one workgroup; 280x192
N_FRAMES = (1, 2, 3, RING, RING + 1, 2 * RING + 1)
N_CLIPS = (1, 3)
PAIRS = ((0, 0), (0, 1), (0, 255), (4, 4), (3, 12), (16, 64), (255, 255))
KINDS = ("noise", "near", "ramp", "flip")
CLIPS, FRAMES = max(N_CLIPS), max(N_FRAMES)
SENTINEL = 0x5B             # tests/stream_probe.py's SENTINEL_B


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def clip(kind, pixels):
    """uint8 (CLIPS, FRAMES, pixels, 3)"""
    rng = np.random.default_rng(1400 + KINDS.index(kind) * 100 + PIXELS.index(pixels))
    shape = (CLIPS, FRAMES, pixels, 3)
    if kind == "noise":
        a = rng.integers(0, 256, shape)
    elif kind == "near":      # a still picture under noise of -6..6: every branch of (4, 4), (3, 12) and (0, 1) is met
        a = rng.integers(0, 256, (CLIPS, 1, pixels, 3)) + rng.integers(-6, 7, shape)
    elif kind == "ramp":      # +1 a frame from a start of the pixel's own, the three channels at different offsets
        a = rng.integers(0, 250, (CLIPS, 1, pixels, 1)) + np.arange(FRAMES)[None, :, None, None] + np.arange(3)
    else:                     # 0 and 255 alternating, the pixel's phase its own: (x - h) * w reaches +-255 * 255
        a = 255 * ((np.arange(FRAMES)[None, :, None, None] + rng.integers(0, 2, (CLIPS, 1, pixels, 1))) & 1) + np.zeros(shape, np.int64)
    return _frozen(np.clip(a, 0, 255).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def want(kind, pixels, pair):
    """the model of the whole block, started at frame 0: (out (CLIPS, FRAMES, pixels, 3), counts uint32 (CLIPS, FRAMES, 3)); the state
    behind frame n - 1 is out[:, n - 1]"""
    out, _, counts = M.hold_clips(clip(kind, pixels), pair[0], pair[1])
    return _frozen(out), _frozen(counts)


# ---- past the first trip of the grid-stride loop -----------------------------------------------------------------------------------

BATCH_PIXELS = 8            # two lanes: one work item a clip
BATCH_FRAMES = 3
BATCH_PAIR = (3, 12)
P = 7                       # clips in the pool
N_SECOND, N_THIRD = GRID_CAP + 1, 2 * GRID_CAP + 1     # the smallest clip counts with a second and with a third trip


def runs_per_clip(pixels):
    return -(-(pixels // LANE_PIXELS) // THREADS)


def trips(n_clips, pixels=BATCH_PIXELS):
    """grid-stride trips the busiest workgroup makes"""
    return -(-n_clips * runs_per_clip(pixels) // GRID_CAP)


def assert_trips(n):
    assert n in (N_SECOND, N_THIRD) and runs_per_clip(BATCH_PIXELS) == 1
    assert trips(N_SECOND - 1) == 1 and trips(N_SECOND) == 2 and trips(N_THIRD - 1) == 2 and trips(N_THIRD) == 3
    assert trips(n) == (3 if n == N_THIRD else 2)
    # the clip a workgroup meets on a later trip is never the pool item it had on an earlier one
    for k in range(1, trips(n)):
        assert (k * GRID_CAP) % P != 0


@functools.lru_cache(maxsize=None)
def pool():
    """uint8 (P, BATCH_FRAMES, BATCH_PIXELS, 3): a still picture under noise of -8..8"""
    rng = np.random.default_rng(1471)
    a = rng.integers(0, 256, (P, 1, BATCH_PIXELS, 3)) + rng.integers(-8, 9, (P, BATCH_FRAMES, BATCH_PIXELS, 3))
    return _frozen(np.clip(a, 0, 255).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def pool_want():
    out, state, counts = M.hold_clips(pool(), *BATCH_PAIR)
    return _frozen(out), _frozen(state), _frozen(counts)


# ---- the full-hold clip --------------------------------------------------------------------------------------------------------------

HOLD_AMPLITUDE, HOLD_PAIR, HOLD_FRAMES, HOLD_SEED = 3, (6, 6), 8, 1481


@functools.lru_cache(maxsize=None)
def still_clip(size=(192, 280)):
    """uint8 (HOLD_FRAMES, H, W, 3): one picture (a two-axis gradient) under uniform noise of -a..a, clamped.  |x_t - x_0| <= 2a for
    every t, so a hold with lo >= 2a gives frame 0 repeated."""
    rng = np.random.default_rng(HOLD_SEED)
    y, x = np.mgrid[0:size[0], 0:size[1]]
    base = np.stack([(x * 255) // (size[1] - 1), (y * 255) // (size[0] - 1), ((x + y) * 255) // (size[0] + size[1] - 2)], axis=-1)
    noise = rng.integers(-HOLD_AMPLITUDE, HOLD_AMPLITUDE + 1, (HOLD_FRAMES,) + base.shape)
    return _frozen(np.clip(base[None] + noise, 0, 255).astype(np.uint8))
