"""include/iivision.h section f14 (the temporal hold) in numpy, frame by frame, with the counts: what csrc/iiv_temporal.hip is held to
byte for byte.  Written from the header's text, per channel with the signed difference and the arithmetic shift, not from the
kernel's rearrangement of it."""
import numpy as np


def weights(lo, hi):
    """w(d) for d = 0..255: int64 (256,)"""
    assert 0 <= lo <= hi <= 255
    d = np.arange(256, dtype=np.int64)
    w = (256 * (d - lo)) // (hi - lo + 1)
    return np.where(d <= lo, 0, np.where(d > hi, 256, w))


def hold(frames, lo, hi, state=None):
    """frames: uint8 (n, ..., 3), one clip -> (out uint8 of the same shape, state uint8 (..., 3) behind the last frame, counts
    uint32 (n, 3) = held, blended, passed).  state=None is `first`: frame 0 passes as it is; otherwise the held frame an earlier
    call returned (left unchanged)."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim >= 2 and frames.shape[-1] == 3
    w_of = weights(lo, hi)
    out = np.empty_like(frames)
    counts = np.zeros((len(frames), 3), np.uint32)
    pixels = int(np.prod(frames.shape[1:-1], dtype=np.int64))
    h = None if state is None else np.asarray(state).astype(np.int64)
    assert h is None or h.shape == frames.shape[1:]
    for t in range(len(frames)):
        x = frames[t].astype(np.int64)
        if h is None:
            h = x.copy()
            counts[t] = (0, 0, pixels)
        else:
            d = np.abs(x - h).max(axis=-1)
            w = w_of[d][..., None]
            h = h + (((x - h) * w + 128) >> 8)      # numpy's >> on int64 is arithmetic
            counts[t] = ((d <= lo).sum(), ((d > lo) & (d <= hi)).sum(), (d > hi).sum())
        assert h.min() >= 0 and h.max() <= 255
        out[t] = h
    if h is None:   # no frames and no state: nothing is held yet
        return out, None, counts
    return out, h.astype(np.uint8), counts


def hold_clips(frames, lo, hi, states=None):
    """frames: uint8 (c, n, ..., 3) -> (out, states (c, ..., 3), counts (c, n, 3)); n >= 1"""
    res = [hold(frames[k], lo, hi, None if states is None else states[k]) for k in range(len(frames))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res])
