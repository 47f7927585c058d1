"""What the encoder-vs-oracle GPU tests share: the inputs, the encoder under test, the oracle's run, and the checks.

One copy of each step -- build an encoder from the device's tables with some options, seed its generators, put frames on the
device, run a schedule through the oracle, compare opcodes and state -- so that which fields a test compares is a decision
made here, not a matter of which file it was copied from.  Both state checkers read the device through enc.get_state only:
tests/test_encode_harness_host.py drives them on the CPU with a stand-in and shows that each compared field bites."""

import ctypes as C

import numpy as np

import mt_model

DHGR = 1


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def seed_states(O, seed_py, seed_np):
    """(625 words of random.seed(seed_py), 625 words of np.random.seed(seed_np))"""
    return O.mt_seed_py(seed_py).state_words(), O.mt_seed_np(seed_np).state_words()


def next_draws(O, words, n, high):
    """the next n draws of a generator in state `words`: random.getrandbits(8) (high) or np.random.randint(0, 256)"""
    m = O.MT()
    m.set_state_words(words)
    L = O.lib()
    f = L.orc_py_getrandbits8 if high else L.orc_np_randint256
    return [f(C.byref(m)) for _ in range(n)]


def synth(mode, n_frames, seed, coherent=False):
    """(n_frames, 2, 32, 256) iid bytes, screen holes zero; coherent: 90 % of a frame's bytes are the frame's before.
    Oracle expectations hang on these bytes: test_encode_harness_host.py pins them by hash."""
    holes = (np.arange(256) & 127) >= 120
    rng = np.random.default_rng(seed)
    hi = 128 if mode == 1 else 256
    banks = 2 if mode == 1 else 1
    fr = np.zeros((n_frames, 2, 32, 256), np.uint8)
    prev = None
    for f in range(n_frames):
        cur = []
        for b in range(banks):
            new = rng.integers(0, hi, (32, 256), dtype=np.uint8)
            if coherent and prev is not None:
                new = np.where(rng.random((32, 256)) < 0.9, prev[b], new)
            new[:, holes] = 0
            cur.append(new)
        prev = cur
        for b in range(banks):
            fr[f, b] = cur[b]
    return fr


def device_frames(mode, frames_list):
    """streams' (n_frames, banks, 32, 256) arrays -> (main, aux | None) device tensors (n, max n_frames, 32, 256); a stream
    with fewer frames is filled up with copies of its last one (its schedule never names them)"""
    import torch
    nf = max(len(f) for f in frames_list)
    fr = np.stack([np.concatenate([f] + [f[-1:]] * (nf - len(f))) for f in frames_list])
    fm = torch.from_numpy(np.ascontiguousarray(fr[:, :, 0])).cuda()
    fa = torch.from_numpy(np.ascontiguousarray(fr[:, :, 1])).cuda() if mode == DHGR else None
    return fm, fa


def segments(sched):
    """(frame, is_aux, n) -> (frame, is_aux, 1, n): every entry starts a generator; four-tuples pass through"""
    return [tuple(int(x) for x in (g if len(g) == 4 else (g[0], g[1], 1, g[2]))) for g in sched]


def tags(archive):
    """the case names of an archive whose arrays are called tag/key"""
    return sorted(set(k.split("/")[0] for k in archive.files))


def recorded(archive, tag):
    """one case of a tag/key archive (g3, g8) as the mapping check_recorded_state takes"""
    class View:
        def __getitem__(self, key):
            return archive[tag + "/" + key]
    return View()


# ---- the encoder under test -----------------------------------------------------------------------------------------------

_LEAVE = object()       # an option that was not named keeps the library's default: no call is made for it


def make_encoder(native, device_tables, mode, pal=5, n_streams=1, *, dw=_LEAVE, kernel=_LEAVE, prefix=_LEAVE, fourth=_LEAVE,
                 joint=_LEAVE, dm=True, rng=None, O=None):
    """An encoder of n_streams streams over the tables of (mode, pal).

    device_tables: the fixture, or (table, store table, diff matrix) of a test that builds its own.  dm=False leaves the diff
    matrix out: a table-only encoder (table gathers, workgroup kernel).  The options that were named are applied in this
    order, the others not at all: dw (set_diff_weights_mode), kernel (set_greedy_kernel), prefix (set_prefix_sort), fourth
    (set_fourth_offset), joint (set_content_choice).  rng: per stream (py_words, np_words), or (seed_py, seed_np) together
    with O; uploaded with set_state_all."""
    if isinstance(device_tables, tuple):
        t, s, matrix = device_tables
    else:
        t, s = device_tables.get(mode, pal)
        matrix = device_tables.dm[(mode, pal)]
    enc = native.Encoder(mode, t, s, n_streams, dm=matrix) if dm else native.Encoder(mode, t, s, n_streams)
    for value, put in ((dw, enc.set_diff_weights_mode), (kernel, enc.set_greedy_kernel), (prefix, enc.set_prefix_sort),
                       (fourth, enc.set_fourth_offset), (joint, enc.set_content_choice)):
        if value is not _LEAVE:
            put(value)
    if rng is not None:
        assert len(rng) == n_streams, (len(rng), n_streams)
        st = [seed_states(O, a, b) if np.ndim(a) == 0 else (a, b) for a, b in rng]
        enc.set_state_all(native.STATE_RNG_PY, np.stack([py for py, _ in st]))
        enc.set_state_all(native.STATE_RNG_NP, np.stack([npw for _, npw in st]))
    return enc


def seeded_batch(device_tables, mode, n_streams):
    """a stream_batch.StreamBatch of n_streams streams on seeds (s + 1, s + 11): the render tests' measured encoder and its twin"""
    import stream_batch
    table, store = device_tables.get(mode)
    return stream_batch.StreamBatch(mode, table, store, n_streams, seeds=[(s + 1, s + 11) for s in range(n_streams)],
                                    dm=device_tables.dm[(mode, 5)])


# the items of native.Encoder.get_state two such twins are compared in
STATE_NAMES = ["STATE_MEM_MAIN", "STATE_MEM_AUX", "STATE_UP_MAIN", "STATE_UP_AUX", "STATE_RNG_PY", "STATE_RNG_NP", "STATE_OUT_OF_WORK",
               "STATE_COUNTERS"]


# ---- the oracle's side ----------------------------------------------------------------------------------------------------

def oracle_run(O, oracle_tables, mode, pal, frames, sched, seeds_or_words, *, fourth=False, joint=False, init=None,
               per_opcode=False):
    """One stream through the oracle -> (Video, opcodes).  frames: (n_frames, 2, 32, 256); sched: three- or four-tuples
    (segments); seeds_or_words: (seed_py, seed_np), or both generators' 625 words; init(v) runs before the first frame.
    per_opcode: one opcode per call -> (Video, opcodes, steps, seg_np), the draws of `random` per opcode and of `np.random`
    per restart (the reference's generator is lazy: its prologue runs in the first next())."""
    a, b = seeds_or_words
    if np.ndim(a) == 0:
        v = O.Video(mode, oracle_tables.get(mode, pal), seed_py=a, seed_np=b)
    else:
        v = O.Video(mode, oracle_tables.get(mode, pal))
        v.rng_py().set_state_words(a)
        v.rng_np().set_state_words(b)
    if joint:
        v.set_joint(joint)
    if fourth:
        v.set_fourth_offset(fourth)
    if init:
        init(v)
    ops, steps, seg_np = [], [], []
    for (f, ia, restart, n) in segments(sched):
        if restart:
            before = v.draws()[1]
            v.encode_frame(frames[f, 0], frames[f, 1] if mode == DHGR else None, ia)
        if not per_opcode:
            if n:
                ops.append(v.next(n))
            continue
        for k in range(n):
            d0 = v.draws()[0]
            ops.append(v.next(1))
            if restart and k == 0:
                seg_np.append(v.draws()[1] - before)
            steps.append(v.draws()[0] - d0)
    ops = np.concatenate(ops) if ops else np.zeros((0, 6), np.uint8)
    return (v, ops, steps, seg_np) if per_opcode else (v, ops)


class State:
    """what check_oracle_state compares, held as copies: mem and up per bank, packed, out_of_work, draws, py, np"""

    def __init__(self, **fields):
        assert sorted(fields) == sorted(FIELDS), sorted(fields)
        self.__dict__.update(fields)


def oracle_state(v, mode):
    """a Video's State, for a test that keeps it while the Video runs on (or for hundreds of runs)"""
    banks = range(mode + 1)
    return State(
        mem=[v.memory(b).copy() for b in banks], up=[v.update_priority(b).copy() for b in banks], packed=v.packed.copy(),
        out_of_work=[int(v.out_of_work(0)), int(v.out_of_work(1))], draws=tuple(v.draws()),
        py=v.rng_py().state_words(), np=v.rng_np().state_words())


# ---- the checks -----------------------------------------------------------------------------------------------------------

def first_difference(got, want, tag=""):
    """the first row in which two opcode arrays of one shape differ, or None"""
    assert got.shape == want.shape, "%s: opcodes of shape %s, want %s" % (tag, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    return None if len(bad) == 0 else int(bad[0])


def check_ops(got, want, tag):
    bad = first_difference(got, want, tag)
    assert bad is None, "%s: first opcode mismatch at %d of %d: got %s want %s" % (tag, bad, len(want), got[bad], want[bad])


def check_recorded_state(native, O, enc, i, rec, tag):
    """stream i against a recording of the reference: mem, up and packed per bank, out_of_work, four next draws of each
    generator.  rec: a mapping with mem_main, up_main, packed, mem_aux, up_aux, out_of_work, py_next, np_next and meta
    (meta[0]: the mode; the aux keys are read in DHGR only)."""
    def same(what, key):
        assert np.array_equal(enc.get_state(what, i), rec[key]), "%s: %s differs from the recording" % (tag, key)
    same(native.STATE_MEM_MAIN, "mem_main")
    same(native.STATE_UP_MAIN, "up_main")
    same(native.STATE_PACKED, "packed")
    if int(rec["meta"][0]) == DHGR:
        same(native.STATE_MEM_AUX, "mem_aux")
        same(native.STATE_UP_AUX, "up_aux")
    got = enc.get_state(native.STATE_OUT_OF_WORK, i).tolist()
    assert got == rec["out_of_work"].tolist(), "%s: out_of_work %s, recorded %s" % (tag, got, rec["out_of_work"].tolist())
    for what, key, high in ((native.STATE_RNG_PY, "py_next", True), (native.STATE_RNG_NP, "np_next", False)):
        got = next_draws(O, enc.get_state(what, i), 4, high)
        assert got == rec[key].tolist(), "%s: %s %s, recorded %s" % (tag, key, got, rec[key].tolist())


def same_stream(got, want, what):
    """two generator states name one stream: equal in mt_model's canonical form (raw index 624 is index 0 of the next block)"""
    g, w = mt_model.canonical(got), mt_model.canonical(want)
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, "%s: canonical state differs in %d words, first at %d (624 = the index): got %d (raw index %d), want %d" % (
        what, len(bad), bad[0], g[bad[0]], got[624], w[bad[0]])


FIELDS = ("mem", "up", "packed", "out_of_work", "draws", "py", "np")


def check_oracle_state(native, enc, i, v, mode, tag, fields=FIELDS):
    """stream i against the oracle's Video (or a State: oracle_state's copy of one, or device_state's of an earlier moment of
    the stream itself): both banks' mem and up (HGR: the one bank),
    packed, out_of_work, the draw counters of random and np.random, and both generators in full.  fields: a call site whose
    stricter check turned up a finding names the subset it had before.  Returns what it read from the device."""
    assert set(fields) <= set(FIELDS), fields
    want = v if isinstance(v, State) else oracle_state(v, mode)
    got = {}
    for b in range(mode + 1):
        if "mem" in fields:
            got.setdefault("mem", []).append(enc.get_state(native.STATE_MEM_MAIN + b, i))
            assert np.array_equal(got["mem"][b], want.mem[b]), "%s: mem of bank %d differs from the oracle" % (tag, b)
        if "up" in fields:
            got.setdefault("up", []).append(enc.get_state(native.STATE_UP_MAIN + b, i))
            assert np.array_equal(got["up"][b], want.up[b]), "%s: up of bank %d differs from the oracle" % (tag, b)
    if "packed" in fields:
        got["packed"] = enc.get_state(native.STATE_PACKED, i)
        assert np.array_equal(got["packed"], want.packed), "%s: packed differs from the oracle" % tag
    if "out_of_work" in fields:
        got["out_of_work"] = enc.get_state(native.STATE_OUT_OF_WORK, i).tolist()
        assert got["out_of_work"] == want.out_of_work, "%s: out_of_work %s, oracle %s" % (tag, got["out_of_work"], want.out_of_work)
    if "draws" in fields:
        got["draws"] = tuple(int(x) for x in enc.get_state(native.STATE_COUNTERS, i)[:2])
        assert got["draws"] == want.draws, "%s: draws (random, np.random) %s, oracle %s" % (tag, got["draws"], want.draws)
    if "py" in fields:
        got["py"] = enc.get_state(native.STATE_RNG_PY, i)
        same_stream(got["py"], want.py, "%s: py (random)" % tag)
    if "np" in fields:
        got["np"] = enc.get_state(native.STATE_RNG_NP, i)
        same_stream(got["np"], want.np, "%s: np (np.random)" % tag)
    return got


def device_state(native, enc, i, mode):
    """stream i's State as the device holds it now: what a later check_oracle_state finds unchanged, or not"""
    return State(mem=[enc.get_state(native.STATE_MEM_MAIN + b, i) for b in range(mode + 1)],
                 up=[enc.get_state(native.STATE_UP_MAIN + b, i) for b in range(mode + 1)],
                 packed=enc.get_state(native.STATE_PACKED, i), out_of_work=enc.get_state(native.STATE_OUT_OF_WORK, i).tolist(),
                 draws=tuple(int(x) for x in enc.get_state(native.STATE_COUNTERS, i)[:2]),
                 py=enc.get_state(native.STATE_RNG_PY, i), np=enc.get_state(native.STATE_RNG_NP, i))


def screen_error(native, device_tables, mode, enc, frames, last, n):
    """sum of Bitmap.diff_weights(current screen -> target frame `last`) over both banks, per stream"""
    t, _ = device_tables.get(mode, 5)
    tot = np.zeros(n, np.int64)
    for i in range(n):
        cur_m = enc.get_state(native.STATE_MEM_MAIN, i)
        cur_a = enc.get_state(native.STATE_MEM_AUX, i) if mode == 1 else None
        src = native.pack(mode, cur_m[None], cur_a[None] if cur_a is not None else None)
        tgt = native.pack(mode, frames[i][last, 0][None], frames[i][last, 1][None] if mode == 1 else None)
        for ia in ((0, 1) if mode == 1 else (0,)):
            tot[i] += int(native.diff_weights(mode, t, src, tgt, ia).sum())
    return tot
