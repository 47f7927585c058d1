"""Diff matrices at the encoder's 11-bit limit, the clips that reach it, and the schedules run over them: shared by
tests/test_limit_matrices_host.py (the oracle alone: do the inputs reach the limit?) and tests/test_gpu_limit_matrices.py
(the device against the oracle).  Plain functions and constants, no fixtures.

iiv_build_table / iiv_build_store_table / iiv_encoder_create take any 16x16 integer diff matrix dm with
max(dm) * MASKED_DOTS <= 2047: max(dm) up to 204 for DHGR (10 dots, values up to 2040) and 113 for HGR (18 dots, values up to
2034).  Everything here sits exactly there."""
import numpy as np

HGR, DHGR = 0, 1
MODES = [DHGR, HGR]
MAX_VALUE = 2047                      # what the encoder's key fields hold (csrc/iiv_stream.h)
DOTS = {DHGR: 10, HGR: 18}            # MASKED_DOTS (the tests hold it to O.masked_dots)
MATRICES = ["flat", "two_level", "spread", "lower_wins"]
HOLES = (np.arange(256) & 127) >= 120
WHITE = {DHGR: 0x7f, HGR: 0xff}
UP_BIG = 0xffff                       # the kernels' 16-bit priority copy says "see the int32 entry" with this value

_dm = {}


def limit(mode):
    """L: the largest entry a diff matrix of this mode may hold"""
    return MAX_VALUE // DOTS[mode]


def matrix(mode, name):
    """(256,) int32, zero diagonal (read-only, cached).
    flat:       every off-diagonal entry is L -- the largest table value, diff weight and delta.
    two_level:  symmetric, entries 0..3 except thirty seeded pairs at L, (0, 15) among them -- no metric: a path over cheap
                pairs undercuts the dear ones, which drives the terms the store table's and the pair-term table's biases
                exist for (r0 - s, 1 - s) as far negative as the formats allow.
    spread:     symmetric, uniform in [0, L], dm[3, 9] = dm[9, 3] = 0 (two identical colours).
    lower_wins: NOT symmetric; strict lower triangle uniform in [L / 2, L], upper in 0..3 -- the table builders take the
                lower triangle (make_data_tables.py:81-87)."""
    if (mode, name) in _dm:
        return _dm[(mode, name)]
    L = limit(mode)
    rng = np.random.default_rng(9000 + MATRICES.index(name))
    if name == "flat":
        dm = np.full((16, 16), L, np.int32)
    elif name == "two_level":
        dm = np.triu(rng.integers(0, 4, (16, 16), dtype=np.int32), 1)
        pairs = [(a, b) for a in range(16) for b in range(a + 1, 16) if (a, b) != (0, 15)]
        for k in rng.choice(len(pairs), 29, replace=False):
            dm[pairs[k]] = L
        dm[0, 15] = L
        dm = dm + dm.T
    elif name == "spread":
        dm = np.triu(rng.integers(0, L + 1, (16, 16), dtype=np.int32), 1)
        dm = dm + dm.T
        dm[3, 9] = dm[9, 3] = 0
        dm[0, 15] = dm[15, 0] = L    # (the limit itself, whatever the draw)
    elif name == "lower_wins":
        dm = np.tril(rng.integers(L // 2, L + 1, (16, 16), dtype=np.int32), -1) + np.triu(rng.integers(0, 4, (16, 16), dtype=np.int32), 1)
        dm[1, 0] = L                 # (the limit itself, whatever the draw)
    else:
        raise KeyError(name)
    np.fill_diagonal(dm, 0)
    dm = np.ascontiguousarray(dm.reshape(256).astype(np.int32))
    dm.setflags(write=False)
    _dm[(mode, name)] = dm
    return dm


def over_limit(mode):
    """L + 1 everywhere off the diagonal: one more than any of the formats was sized for"""
    dm = np.full((16, 16), limit(mode) + 1, np.int32)
    np.fill_diagonal(dm, 0)
    return np.ascontiguousarray(dm.reshape(256))


# ---- clips: (frames, 2, 32, 256) uint8, screen holes zero, DHGR bytes with bit 7 clear, HGR's aux bank unused (zero)

def frame(mode, name):
    banks = 2 if mode == DHGR else 1
    f = np.zeros((2, 32, 256), np.uint8)
    w = WHITE[mode]
    if name == "white":
        f[:banks] = w
    elif name == "half":               # byte columns 0..63 and 128..191 white, the rest black
        f[:banks, :, (np.arange(256) & 64) == 0] = w
    elif name == "stripes":            # alternate bytes white and black
        f[:banks, :, 0::2] = w
    elif name == "noise":
        f[:banks] = np.random.default_rng(4242 + mode).integers(0, w + 1, (banks, 32, 256), dtype=np.uint8)
    elif name != "black":
        raise KeyError(name)
    f[:, :, HOLES] = 0
    return f


CLIP = ["white", "half", "noise", "black", "stripes"]


def clip(mode, names=CLIP):
    return np.ascontiguousarray(np.stack([frame(mode, n) for n in names]))


# ---- schedules: lists of (frame of clip(mode), is_aux, restart, n_ops)

def encode_schedule(mode, cap=None):
    """white, white (other bank), half, noise (other bank), black through 2200 opcodes -- past the sorted list into the
    re-queued bag --, stripes and a continuation of that generator.  cap: every count cut to at most that many."""
    aux = 1 if mode == DHGR else 0
    sched = [(0, 0, 1, 300), (0, aux, 1, 250), (1, 0, 1, 400), (2, aux, 1, 300), (3, 0, 1, 2200), (4, 0, 1, 300), (4, 0, 0, 200)]
    return [(f, a, r, min(k, cap) if cap else k) for (f, a, r, k) in sched]


# ---- a step that STORES a value at the limit
# What a step leaves at a secondary offset (video.py:166-170) is the best of its page's candidates, and a picture-sized target
# always offers better ones than a store that mends one dot of ten (18): on the clip above such values stay below half the
# limit.  Here the candidates are made: on a screen of bytes SCREEN every page has one byte A whose target is CONTENT and four
# bytes B whose target is OTHER, chosen (by search over the flat matrix's table) so that every dot of a B is wrong on the
# screen and CONTENT there mends exactly one, while it makes every other byte of the page worse.  A waits through one short
# generator, which doubles its priority past any B's; the generator that then sees the Bs takes the waiting As first, and
# each of them finds nothing better for its two (three) extra offsets than Bs at delta -L: the value stored is L * dots - L.
STORE = {DHGR: dict(screen=0x00, content=0x76, other=0x4b), HGR: dict(screen=0xe2, content=0xdd, other=0x18)}
STORE_A, STORE_B = 10, (40, 51, 60, 71)      # offsets on every page (both parities among the Bs)
STORE_PRE = 3000                              # opcodes that put SCREEN on a black screen and run out of work (7680 bytes, three a step)


def store_clip(mode):
    """(3, 2, 32, 256): the screen, the screen with the As pending, the same with the Bs pending too (main bank)"""
    s = STORE[mode]
    ctx = np.zeros((2, 32, 256), np.uint8)
    ctx[:2 if mode == DHGR else 1] = s["screen"]
    ctx[:, :, HOLES] = 0
    wait = ctx.copy()
    wait[0, :, STORE_A] = s["content"]
    both = wait.copy()
    both[0, :, list(STORE_B)] = s["other"]
    return np.ascontiguousarray(np.stack([ctx, wait, both]))


def store_schedule(mode):
    """bring the screen up (nothing to do for a black one), let 4 of the 32 As go while the others wait, then the Bs"""
    pre = [(0, b, 1, STORE_PRE) for b in ((0, 1) if mode == DHGR else (0,))] if STORE[mode]["screen"] else []
    return pre + [(1, 0, 1, 4), (2, 0, 1, 64)]


CROSS_ROUNDS, CROSS_FIRST = 40, 32    # rounds on the white target; the round (from 0) that takes a priority past 65535


def crossing_schedule(mode):
    """Three parts, the priorities to be read after each.  Forty rounds of 8 opcodes on a constant white target: a byte that
    waits gains the largest diff weight every round, 32 * 2040 = 65280 (32 * 2034 = 65088) after round 31 and past 65535
    with round 32.  A generator adds to its own bank only, so in DHGR a round is a generator on each bank and both banks
    cross in round 32.  Then two generators of 300 opcodes on the noise frame, which order by the priorities left behind."""
    banks = (0, 1) if mode == DHGR else (0,)
    rounds = [[(0, b, 1, 8) for b in banks] for _ in range(CROSS_ROUNDS)]
    flat = lambda rs: [g for r in rs for g in r]
    return [flat(rounds[:CROSS_FIRST]), flat(rounds[CROSS_FIRST:CROSS_FIRST + 1]),
            flat(rounds[CROSS_FIRST + 1:]) + [(2, 0, 1, 300), (2, banks[-1], 1, 300)]]


def oracle_run(O, mode, table, frames, sched, seeds=(5, 6), fourth=False, joint=False, after=None):
    """The oracle over a schedule -> (its Video, opcodes).  after(v, segment index) is called behind every segment."""
    v = O.Video(mode, table, seed_py=seeds[0], seed_np=seeds[1])
    v.set_fourth_offset(fourth)
    v.set_joint(joint)
    ops = []
    for i, (f, ia, restart, k) in enumerate(sched):
        if restart:
            v.encode_frame(frames[f, 0], frames[f, 1] if mode == DHGR else None, ia)
        ops.append(v.next(k))
        if after is not None:
            after(v, i)
    return v, np.concatenate(ops)
