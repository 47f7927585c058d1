"""What the speaker tests share (tests/test_gpu_speaker.py, tests/test_gpu_speaker_batches.py, tests/test_speaker_batches_host.py):
the batch of nine counts with its three kinds of ticks, the pool of the grid-stride batches, the constants mirrored from
csrc/iiv_speaker.hip, and the model's samples of each, computed once and shared read-only."""
import functools

import numpy as np

import speaker_model as M

# ---- the case grid ---------------------------------------------------------------------------------------------------------------

COUNTS = (0, 1, 2, 290, 291, 292, 583, 584, 900)      # one stream each; ACKs follow opcodes 290 and 582
STRIDE = 900
DECIMS = (1, 7, 23, 64, 73)
ORDERS = (1, 3, 4)
GAINS = (0, 16384, 32767)
KINDS = ("random", "extremes", "odd")
FILL_TICK = 0xFF            # behind a stream's own count: no tick, so a kernel that reads past the count raises the flag
SENTINEL = 0x5B5B           # what an unwritten sample holds (both bytes tests/stream_probe.py's SENTINEL_B)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ticks(kind):
    """uint8 (9, STRIDE): row s holds COUNTS[s] ticks of the kind and FILL_TICK behind them"""
    rng = np.random.default_rng({"random": 1301, "extremes": 1302, "odd": 1303}[kind])
    t = np.full((len(COUNTS), STRIDE), FILL_TICK, np.uint8)
    for s, n in enumerate(COUNTS):
        if kind == "random":
            t[s, :n] = rng.integers(0, 32, n) * 2 + 4
        elif kind == "extremes":
            t[s, :n] = 4 if s % 2 else 66
        else:
            t[s, :n] = np.where(rng.integers(0, 2, n) == 1, 22, 40)
    return _frozen(t)


@functools.lru_cache(maxsize=None)
def accumulated(kind, s, decim, order):
    return _frozen(M.accumulate(ticks(kind)[s, :COUNTS[s]], decim, order))


def want(kind, s, decim, order, gain):
    """the model's samples of stream s: int16 (M(s),)"""
    v = (accumulated(kind, s, decim, order) * gain) // (decim ** order)
    return np.clip(v, -32768, 32767).astype(np.int16)


# ---- past the first trip of the grid-stride loop -----------------------------------------------------------------------------------

# mirrored from csrc/iiv_speaker.hip; tests/test_speaker_batches_host.py reads them from its text and fails if they moved
RUN = 2048                  # constexpr int kSpeakerRun = 2048: samples of one work item
GRID_CAP = 2048             # constexpr int kSpeakerGridCap = 2048: workgroups of a launch
THREADS, PER_THREAD = 256, 8

BATCH_DECIM = 73            # one sample a period: the fewest samples an opcode can have
BATCH_STRIDE = 2040         # opcodes a row holds: 2052 periods = 2052 samples at decim 73 = two runs a stream
P = 7                       # items in the pool
N_SECOND, N_THIRD = 1025, 2049   # the smallest batches with a second and with a third trip
# the pool's counts: two runs, exactly one run, one run and one sample, a short stream, none, all 2040, and one with a short second run
POOL_COUNTS = (2040, 2036, 2037, 300, 0, 2040, 2039)


def runs_per_stream():
    return -(-M.sample_count(BATCH_STRIDE, BATCH_DECIM) // RUN)


def trips(n_streams):
    """grid-stride trips the busiest workgroup makes for a batch of n_streams rows of BATCH_STRIDE ticks"""
    return -(-n_streams * runs_per_stream() // GRID_CAP)


def assert_trips(n):
    assert n in (N_SECOND, N_THIRD)
    assert M.sample_count(BATCH_STRIDE, BATCH_DECIM) == 2052 and runs_per_stream() == 2
    assert trips(N_SECOND - 1) == 1 and trips(N_SECOND) == 2 and trips(N_THIRD - 1) == 2 and trips(N_THIRD) == 3
    assert trips(n) == (3 if n == N_THIRD else 2)
    # the stream a workgroup meets on a later trip is never the pool item it had on an earlier one: GRID_CAP items are 1024
    # streams on, and 1024 = 2 (mod 7), 2048 = 4 (mod 7)
    per_trip = GRID_CAP // runs_per_stream()
    assert per_trip * runs_per_stream() == GRID_CAP
    for k in range(1, trips(n)):
        assert (k * per_trip) % P != 0
    # the counts meet every way a row's second run can end: absent (M <= RUN), one sample, some, all of the row's 2052
    m = [M.sample_count(c, BATCH_DECIM) for c in POOL_COUNTS]
    assert m == [2052, 2048, 2049, 302, 0, 2052, 2051]


@functools.lru_cache(maxsize=None)
def pool():
    """uint8 (P, BATCH_STRIDE): random legal ticks, FILL_TICK behind each item's own count"""
    rng = np.random.default_rng(1307)
    t = np.full((P, BATCH_STRIDE), FILL_TICK, np.uint8)
    for i, n in enumerate(POOL_COUNTS):
        t[i, :n] = rng.integers(0, 32, n) * 2 + 4
    return _frozen(t)


@functools.lru_cache(maxsize=None)
def pool_want(order, gain):
    """the model's samples of the seven: int16 (P, 2052), SENTINEL behind each item's own M"""
    width = M.sample_count(BATCH_STRIDE, BATCH_DECIM)
    out = np.full((P, width), SENTINEL, np.int16)
    for i, n in enumerate(POOL_COUNTS):
        pcm, bad = M.pcm(pool()[i, :n], BATCH_DECIM, order, gain)
        assert not bad
        out[i, :len(pcm)] = pcm
    return _frozen(out)
