"""Target clips that are NOT tidy -- screen holes that hold bytes, DHGR bytes with bit 7 set -- the schedules run over them,
and the oracle stepped until one of the reference's asserts fires: shared by tests/test_assert_inputs_host.py (the oracle
alone, and the reference's recorded runs: do the inputs do what they are for?) and tests/test_gpu_reference_asserts.py (every
kernel form against the oracle).  Plain functions and constants, no fixtures.

Clips are (frames, 2, 32, 256) uint8 (HGR's aux bank is never read), schedules are lists of (frame, is_aux, restart, n_ops),
every clip belongs to the seed pair in SEEDS and to the tables of palette 5: where a byte sorts depends on both.

What the reference does with such input (video.py):
  :87   asserts that the generator's own memory map is zero in the screen holes -- the TARGET's holes are never looked at:
        :111 zeroes their diff weights, so they are never popped, but the byte at offset 120 / 128 is still the neighbour in
        the windows of offsets 119 / 127's other side, 128 (in DHGR: the other bank's byte).
  :137  asserts that a DHGR content byte is below 0x80 -- at the moment the byte is POPPED.  A byte whose diff weight is 0
        never is, and one that sorts behind the opcode budget is not popped in that budget."""
import ctypes
import re

import numpy as np

HGR, DHGR = 0, 1
MODES = [DHGR, HGR]
HOLES = (np.arange(256) & 127) >= 120
# the columns whose windows hold a hole byte (119 | 120, 127 | 128 and the row's ends) and the holes themselves
HOLE_NEIGHBOURS = np.isin(np.arange(256), [119, 128, 247, 0])
SEEDS = {"clean": (11, 12), "clean2": (13, 14), "dirty_holes": (21, 22), "quiet": (31, 32), "late": (41, 42), "early": (51, 52)}
ERR_PALETTE_BIT = -4                  # the oracle's code of video.py:137 (oracle/iiv_oracle.c: step_heap)
ERR_HOLES, ERR_NEGATIVE = -1, -2      # :87 and :117 (gen_prologue)
MSG_87, MSG_117, MSG_137 = "video.py:87", "video.py:117", "video.py:137"

_BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]])


def banks(mode):
    return (0, 1) if mode == DHGR else (0,)


def picture(mode, seed, n_frames, window=None):
    """Picture-like frames: a grey ramp in moving bars under a 4x4 ordered dither, seven dots a byte (HGR: the palette bit
    from a second, slower field).  Holes zero, DHGR bytes below 0x80.  window = (pages, offsets): everything else black."""
    rng = np.random.default_rng(seed)
    period, speed, slope, phase = int(rng.integers(24, 120)), int(rng.integers(3, 9)), int(rng.integers(-2, 3)), int(rng.integers(0, 120))
    bank, page, off, bit = np.ogrid[0:2, 0:32, 0:256, 0:7]
    x = ((off * 2 + (1 - bank)) if mode == DHGR else off) * 7 + bit
    out = np.zeros((n_frames, 2, 32, 256), np.uint8)
    for f in range(n_frames):
        t = (x + slope * page * 8 + speed * f + phase) % period
        dots = (t * 17) // period > _BAYER[page % 4, x % 4]
        out[f] = (dots << bit).sum(-1).astype(np.uint8)
        if mode == HGR:
            out[f] |= ((((off + page + f) // 9) & 1) << 7).astype(np.uint8)[..., 0]
    if window is not None:
        keep = np.zeros((32, 256), bool)
        keep[window[0], window[1]] = True
        out[:, :, ~keep] = 0
    out[:, :, :, HOLES] = 0
    if mode == HGR:
        out[:, 1] = 0
    return out


def clean(mode, name="clean"):
    """(3, 2, 32, 256): a tidy clip, for the streams beside a bad one"""
    return picture(mode, 100 + SEEDS[name][0], 3)


def clean_schedules(mode):
    """two calls: a restart on each bank and a continuation; a continuation across the calls, then the next frames"""
    aux = 1 if mode == DHGR else 0
    return [(0, aux, 1, 120), (0, 0, 1, 150), (1, 0, 1, 90), (1, 0, 0, 40)], [(1, 0, 0, 30), (1, aux, 1, 100), (2, 0, 1, 70)]


# ---- dirty_holes: the reference accepts it

def dirty_holes(mode, tidy=False):
    """(3, 2, 32, 256), coherent: frame f + 1 keeps nine bytes in ten of frame f.  Every hole byte of both banks is random and
    non-zero, in DHGR half of them with bit 7 set; the hole bytes and the bytes beside them (offsets 119, 128, 247, 0) differ
    from frame to frame (in DHGR: below bit 7), so the windows that hold a hole byte are scored in every generator.
    tidy = True: the same clip with the holes zeroed."""
    rng = np.random.default_rng(77 + mode)
    hi = 127 if mode == DHGR else 255
    frames = picture(mode, 177 + mode, 3)
    for f in range(1, 3):                       # (coherent: only a tenth of the picture moves on)
        keep = rng.random((2, 32, 256)) < 0.9
        frames[f] = np.where(keep, frames[f - 1], frames[f])
    cols = HOLES | HOLE_NEIGHBOURS
    base = rng.integers(0, hi, (2, 32, int(cols.sum())))
    for f in range(3):
        frames[f][:, :, cols] = ((base + 41 * f) % hi + 1).astype(np.uint8)      # 1 .. hi, another value in every frame
    if mode == DHGR:
        top = (rng.random((3, 2, 32, 256)) < 0.5) & HOLES
        frames[top] |= 0x80
    else:
        frames[:, 1] = 0
    if tidy:
        frames[:, :, :, HOLES] = 0
    return np.ascontiguousarray(frames)


def dirty_holes_schedule(mode, cap=None):
    """two frames, both banks in DHGR, one continued generator: 600 opcodes"""
    aux = 1 if mode == DHGR else 0
    sched = [(0, 0, 1, 150), (0, aux, 1, 150), (1, 0, 1, 100), (1, 0, 0, 50), (1, aux, 1, 150)]
    return [(f, a, r, min(k, cap) if cap else k) for (f, a, r, k) in sched]


# ---- quiet_palette_bit: bit 7 where the reference never looks

QUIET_SCHEDULE = [(0, 0, 1, 150), (0, 1, 1, 150), (1, 0, 1, 100), (1, 0, 0, 50), (1, 1, 1, 150)]


def quiet_palette_bit(O, table, mode=DHGR, cap=None, fourth=False, joint=False):
    """(frames, schedule).  Every target byte whose diff weight is 0 when its bank's generator starts -- its masked window
    equals the screen's (or differs by colours at distance 0) -- has bit 7 set: video.py:115 zeroes its priority, it is never
    popped, never chosen as an extra offset (:159), and the reference never asserts.  The first generator runs on a black
    screen, so these are 0x80 bytes in the black parts of a target that is otherwise being drawn.  Which bytes are quiet
    depends on the screen at each generator start: the clip is built along the oracle's run of the schedule with
    SEEDS["quiet"] (and with the given fourth-offset / content-choice options, which change the screen), one generator start
    per frame and bank."""
    assert mode == DHGR
    sched = [(f, a, r, min(k, cap) if cap else k) for (f, a, r, k) in QUIET_SCHEDULE]
    frames = picture(mode, 333, 2, window=(slice(3, 29), slice(8, 250)))
    v = O.Video(mode, table, seed_py=SEEDS["quiet"][0], seed_np=SEEDS["quiet"][1])
    v.set_fourth_offset(fourth)
    v.set_joint(joint)
    for (f, ia, restart, k) in sched:
        if restart:
            dw = O.diff_weights(mode, table, v.packed, O.pack(mode, frames[f, 0], frames[f, 1]), ia)
            frames[f, ia][(dw == 0) & ~HOLES[None, :]] |= 0x80
            v.encode_frame(frames[f, 0], frames[f, 1], ia)
        v.next(k)
    return np.ascontiguousarray(frames), sched


# ---- late_palette_bit: the assert belongs to the launch that pops the byte

LATE_AT = (20, 50)                    # page, offset (main bank) of the byte with bit 7 set
LATE_WINDOW = (slice(4, 12), slice(20, 100))
LATE_INDEX = 230                      # opcodes the main bank's generator yields before the reference asserts (host test)
LATE_SHORT = [(0, 1, 1, 100), (0, 0, 1, LATE_INDEX - 21)]       # ends 21 opcodes in front of the byte: no assert
LATE_MORE = [(0, 0, 0, 60)]           # the same generator, continued past it: the assert fires at opcode 21 of these
LATE_MORE_INDEX = 21
LATE_INDEX_FOURTH = 194               # with the fourth offset a step takes more bytes: the byte's turn comes earlier


def late_short(fourth=False):
    """LATE_SHORT for the run with / without the fourth offset: either ends 21 opcodes in front of the byte"""
    return [LATE_SHORT[0], (0, 0, 1, (LATE_INDEX_FOURTH if fourth else LATE_INDEX) - 21)]


def late_palette_bit(mode=DHGR):
    """(1, 2, 32, 256): a picture in a window of eight pages, and on a page that is otherwise black one byte 0x81 -- a single
    dot, the smallest diff weight there is, and bit 7.  It sorts behind every byte of the picture and no step on its page can
    take it as an extra offset, so the reference pops it -- and asserts -- when the picture's bytes have run out."""
    assert mode == DHGR
    frames = picture(mode, 444, 1, window=LATE_WINDOW)
    frames[0, 0, LATE_AT[0], LATE_AT[1]] = 0x81
    return np.ascontiguousarray(frames)


# ---- early_palette_bit: the assert fires inside the first launch

EARLY_SCHEDULE = [(0, 0, 1, 200)]
# the same behind a short generator on the other bank: round for round the banks of LATE_SHORT and of clean_schedules' first
# call (the LDS-shared form shares one bank's table among the streams of a workgroup)
EARLY_SCHEDULE_BEHIND_AUX = [(1, 1, 1, 30)] + EARLY_SCHEDULE


def early_palette_bit(mode=DHGR, name="clean"):
    """(3, 2, 32, 256): clean(mode, name) with bit 7 set in 64 bytes of frame 0's main bank, two on every page"""
    assert mode == DHGR
    frames = clean(mode, name).copy()
    rng = np.random.default_rng(55)
    ok = np.nonzero(~HOLES)[0]
    for page in range(32):
        frames[0, 0, page, rng.choice(ok, 2, replace=False)] |= 0x80
    return frames


# ---- the oracle, stepped until it asserts

def oracle_video(O, mode, table, seeds, fourth=False, joint=False):
    v = O.Video(mode, table, seed_py=seeds[0], seed_np=seeds[1])
    v.set_fourth_offset(fourth)
    v.set_joint(joint)
    return v


def oracle_steps(v, k):
    """v.next(1) up to k times -> (the opcodes yielded, (n, 6) uint8; the oracle's code: 0, or that of the assert that ended it)"""
    ops = np.zeros((k, 6), np.uint8)
    for i in range(k):
        try:
            ops[i] = v.next(1)[0]
        except AssertionError as e:
            return ops[:i], int(re.search(r"code (-?\d+)", str(e)).group(1))
    return ops, 0


def oracle_run(O, mode, table, frames, sched, seeds, fourth=False, joint=False, v=None):
    """The oracle over a schedule, one opcode a call -> (its Video, the opcodes up to the first assert, the code or 0).
    v: go on with this Video (a later call's schedule)."""
    if v is None:
        v = oracle_video(O, mode, table, seeds, fourth, joint)
    out, code = [np.zeros((0, 6), np.uint8)], 0
    for (f, ia, restart, k) in sched:
        if restart:
            v.encode_frame(frames[f, 0], frames[f, 1] if mode == DHGR else None, ia)
        ops, code = oracle_steps(v, k)
        out.append(ops)
        if code:
            break
    return v, np.concatenate(out), code


def next_draws(O, words, py, n=4):
    """the next n draws of an MT19937 in the state `words` (625 uint32): random.getrandbits(8) / np.random.randint(0, 256)"""
    m = O.MT()
    m.set_state_words(words)
    f = O.lib().orc_py_getrandbits8 if py else O.lib().orc_np_randint256
    return [int(f(ctypes.byref(m))) for _ in range(n)]


def ran(kernel, forms):
    """did the launches run the greedy kernel that was asked for, and no other?  (a silent fall-back must not pass)"""
    others = lambda *keep: sum(n for k, n in forms.items() if k not in keep)
    if kernel is True:                      # one wave per stream: plain or LDS-shared by batch size
        return forms["plain"] + forms["shared"] > 0 and others("plain", "shared") == 0
    key = {"team": "team", "shared": "shared", "plain": "plain", False: "workgroup"}[kernel]
    return forms[key] > 0 and others(key) == 0
