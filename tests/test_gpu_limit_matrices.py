"""GPU: tables and encoder held to the oracle at the 11-bit diff-matrix limit.

Every format behind the encoder is sized for table values up to 2047: iiv_build_table / iiv_build_store_table /
iiv_encoder_create accept any diff matrix with max(dm) * MASKED_DOTS <= 2047 -- max(dm) up to 204 in DHGR, 113 in HGR -- while
the shipped palettes, the mono matrix and test_gpu_tables.py::test_arbitrary_diff_matrices stay at about half of that.  Here
four matrices with max(dm) exactly at the limit (tests/limit_matrices.py) go through the table builders, the store table's
split and narrow forms, the diff-weight checks, iiv_diff_weights / iiv_compute_delta_pages, and an encode in every kernel
form, all against the oracle built from the same matrix; one more than the limit is refused; and priorities cross 16 bits by
the prologue's own additions, read back right at the crossing.  tests/test_limit_matrices_host.py shows on the CPU that
these inputs do reach the limit.  Every comparison is exact."""
import numpy as np
import pytest

import encode_harness as H
import limit_matrices as LM

pytestmark = pytest.mark.gpu

_otab, _dev = {}, {}


def oracle_table(O, mode, name):
    """the oracle's table of a matrix: built once (1.3 s DHGR, 2.9 s HGR), shared, never written to"""
    if (mode, name) not in _otab:
        _otab[(mode, name)] = O.build_table(mode, LM.matrix(mode, name), symmetric=True)
    return _otab[(mode, name)]


def device_tables(native, mode, name):
    """(table, dense store table) of a matrix on the device: built once"""
    if (mode, name) not in _dev:
        dm = LM.matrix(mode, name)
        _dev[(mode, name)] = (native.build_table(mode, dm, True), native.build_store_table(mode, dm))
    return _dev[(mode, name)]


def banks(mode):
    return (0, 1) if mode == LM.DHGR else (0,)


# ---- 1. tables at the limit

PARAMS = [(mode, name) for mode in LM.MODES for name in LM.MATRICES]
# (one function per group of checks: each walks 2.7e8 (DHGR) / 5.4e8 (HGR) entries a few times, and a test stays at seconds)


@pytest.mark.parametrize("mode,name", PARAMS)
def test_table_and_store_table_equal_the_oracles(native, O, mode, name):
    import torch
    top = LM.limit(mode) * O.masked_dots(mode)
    assert O.masked_dots(mode) == LM.DOTS[mode] and top <= LM.MAX_VALUE < top + O.masked_dots(mode)
    otab = oracle_table(O, mode, name)
    table, dense = device_tables(native, mode, name)
    otab_d = torch.from_numpy(otab.view(np.int16)).cuda()
    assert table.shape == otab_d.shape and torch.equal(table, otab_d)                 # every entry
    tmax = int(table.max())                                                           # (equal to the oracle's: none above 2047)
    assert tmax <= top
    if name == "flat":
        assert tmax == top
    # the store table is a gather from the table: the device's equals the gather from the ORACLE's table
    ostore = torch.empty_like(dense)
    native.check(native.lib().iiv_store_table_from_table(mode, native.dptr(otab_d), native.dptr(ostore), native.stream_ptr()))
    assert torch.equal(dense, ostore)


@pytest.mark.parametrize("mode,name", PARAMS)
def test_split_and_narrow_store_tables_are_exact(native, mode, name):
    import torch
    dm = LM.matrix(mode, name)
    _, dense = device_tables(native, mode, name)
    # the split form: expansion with the encoder's own index arithmetic, and the components within their fields
    left, right, exp = native.build_split_store_table(mode, dm)
    assert torch.equal(exp, dense)
    l, r = left.cpu().numpy().view(np.uint32), right.cpu().numpy().view(np.uint32)
    assert int((l & 0xffff).max()) <= 2047 and int((l >> 16).max()) <= 2047 and int((r >> 16).max()) <= 2047
    assert set(np.unique(r & 0xffff)) - set(range(2048)) <= {0x3fff}
    # the narrow form (S = L1 + RF, RF biased): no entry differs, re-read with the kernels' arithmetic
    exp, n_bad = native.build_narrow_store_table(mode, dm, dense)
    assert n_bad == 0 and torch.equal(exp, dense)


def _other(native, mode, name):
    """another limit matrix's table: what a check must NOT call exact"""
    return device_tables(native, mode, LM.MATRICES[(LM.MATRICES.index(name) + 1) % len(LM.MATRICES)])[0]


@pytest.mark.parametrize("mode,name", PARAMS)
def test_split_diff_weight_table_is_exact(native, mode, name):
    dm = LM.matrix(mode, name)
    assert native.check_split_diff_table(mode, dm, device_tables(native, mode, name)[0]) == 0


@pytest.mark.parametrize("mode,name", PARAMS)
def test_diff_weights_as_sums_of_pair_terms_are_exact(native, mode, name):
    """the prologue's pair-term table stores g + a bias, g as low as 1 - s: two_level drives it furthest"""
    dm = LM.matrix(mode, name)
    assert native.check_diff_weight_pieces(mode, dm, device_tables(native, mode, name)[0]) == 0


# (a pass that finds differences costs seconds where an exact one costs a tenth: one function per check and mode)
@pytest.mark.parametrize("mode", LM.MODES)
def test_split_diff_weight_check_can_fail(native, mode):
    assert native.check_split_diff_table(mode, LM.matrix(mode, "flat"), _other(native, mode, "flat")) > 0


@pytest.mark.parametrize("mode", LM.MODES)
def test_pair_term_check_can_fail(native, mode):
    assert native.check_diff_weight_pieces(mode, LM.matrix(mode, "flat"), _other(native, mode, "flat")) > 0


# ---- 2. one over the limit is refused

@pytest.mark.parametrize("mode", LM.MODES)
def test_one_over_the_limit_is_refused(native, mode):
    over = LM.over_limit(mode)
    assert int(over.max()) * LM.DOTS[mode] > LM.MAX_VALUE >= (int(over.max()) - 1) * LM.DOTS[mode]
    with pytest.raises(native.IIVError):
        native.build_table(mode, over, True)
    with pytest.raises(native.IIVError):
        native.build_store_table(mode, over)
    table, dense = device_tables(native, mode, "flat")
    with pytest.raises(native.IIVError):
        native.Encoder(mode, table, dense, 1, dm=over)
    native.Encoder(mode, table, dense, 1, dm=LM.matrix(mode, "flat")).close()       # (the limit itself is taken)


# ---- 3. iiv_diff_weights / iiv_compute_delta_pages at the limit

@pytest.mark.parametrize("name", ["flat", "two_level"])
@pytest.mark.parametrize("mode", LM.MODES)
def test_diff_weights_and_delta_pages_at_the_limit(native, O, mode, name):
    otab = oracle_table(O, mode, name)
    table, _ = device_tables(native, mode, name)
    top = LM.limit(mode) * LM.DOTS[mode]
    packed = {n: O.pack(mode, *LM.frame(mode, n)) for n in ("black", "white", "half", "stripes")}
    pages = np.repeat([0, 3, 31], 4).astype(np.int32)
    contents = np.tile([0, LM.WHITE[mode], 0x55, 0x2a], 3).astype(np.int32)
    seen_lo, seen_hi = 0, 0
    for src, tgt in (("black", "white"), ("black", "half"), ("white", "stripes")):
        for ia in banks(mode):
            want = O.diff_weights(mode, otab, packed[src], packed[tgt], ia)
            got = native.diff_weights(mode, table, packed[src], packed[tgt], ia)
            assert np.array_equal(got, want), (src, tgt, ia)
            if name == "flat" and (src, tgt) == ("black", "white"):
                assert int(got.max()) == top
            want_d = np.stack([O.compute_delta_page(mode, otab, packed[tgt], int(p), int(c), want[p], ia) for p, c in zip(pages, contents)])
            got_d = native.compute_delta_pages(mode, table, packed[tgt], pages, contents, want[pages], ia)
            assert np.array_equal(got_d, want_d), (src, tgt, ia)
            seen_lo, seen_hi = min(seen_lo, int(got_d.min())), max(seen_hi, int(got_d.max()))
    if name == "flat":                       # the largest deltas either way (HGR's largest positive one is 1808)
        assert seen_lo == -top and (seen_hi == top if mode == LM.DHGR else seen_hi >= top - 2 * LM.limit(mode))


# ---- 4. encode at the limit, every kernel form

# (greedy kernel, diff-weight mode): test_arbitrary_diff_matrices' pairing, extended until every kernel meets two modes
KERNEL_FORMS = [("team", True), ("team", "split"), (True, "split"), (True, False), ("plain", True), ("plain", False),
                ("shared", False), ("shared", "split"), (False, True), (False, "split")]
FOURTH_KERNELS = ["team", "shared", True]
JOINT_FORMS = [(True, False), (True, True), ("split", False), ("split", True)]      # (content choice, fourth offset)


def _ran(kernel, forms):
    """did the launches run the form that was asked for, and no other?  (a silent fall-back must not pass)"""
    others = lambda *keep: sum(n for k, n in forms.items() if k not in keep)
    if kernel is True:                      # one wave per stream: its plain form for a single stream
        return forms["plain"] + forms["shared"] > 0 and others("plain", "shared") == 0
    key = {"team": "team", "shared": "shared", "plain": "plain", False: "workgroup"}[kernel]
    return forms[key] > 0 and others(key) == 0


def _device_run(native, O, mode, name, frames, parts, kernel=None, dw=None, fourth=False, joint=False, seeds=(5, 6), write_back=()):
    """One encoder stream over the parts of a schedule -> (opcodes, [priorities of every bank after each part], the encoder
    behind the last part -- _compare reads its state and closes it --, None, launch forms).  Reading the priorities runs materialise_up_kernel (16-bit copy ->
    int32 array); after the parts listed in write_back exactly what was read is written back with set_state, which runs
    materialise_up_kernel, the copy, and compact_up_kernel (int32 array -> 16-bit copy): nothing is planted, the kernels
    after it read what compact_up_kernel left."""
    named = {k: v for k, v in (("kernel", kernel), ("dw", dw)) if v is not None}
    enc = H.make_encoder(native, device_tables(native, mode, name) + (LM.matrix(mode, name),), mode, fourth=fourth, joint=joint,
                         rng=[seeds], O=O, **named)
    enc.profile(True)
    fm, fa = H.device_frames(mode, [frames])
    ops, ups = [], []
    for part in parts:
        got = enc.encode(fm, fa, part)
        enc.check()
        ops.append(got.cpu().numpy()[0])
        ups.append([enc.get_state(native.STATE_UP_MAIN + b) for b in banks(mode)])
        if len(ups) - 1 in write_back:
            for b in banks(mode):
                enc.set_state(native.STATE_UP_MAIN + b, ups[-1][b])
    return np.concatenate(ops), ups, enc, None, enc.launch_forms()


def _compare(native, mode, tag, dev, v, want_ops, want_ups=None):
    ops, ups, enc, _, _ = dev
    H.check_ops(ops, want_ops, str(tag))
    for b in banks(mode):
        for i, w in enumerate(want_ups or ()):
            assert np.array_equal(ups[i][b], w[b]), (tag, "priorities after part", i, "bank", b)
    H.check_oracle_state(native, enc, 0, v, mode, str(tag))
    enc.close()


@pytest.mark.parametrize("name", LM.MATRICES)
@pytest.mark.parametrize("mode", LM.MODES)
def test_encode_at_the_limit_in_every_kernel_form(native, O, mode, name):
    """white, half, noise, black (2200 opcodes: through the list and the bag, out of work), stripes and a continued
    generator: opcodes, priorities, memory and draw counters of every greedy kernel x diff-weight mode, of the fourth offset
    and of both joint content choices equal the oracle's -- and the kernel asked for is the one that ran."""
    otab = oracle_table(O, mode, name)
    frames = LM.clip(mode)
    sched = LM.encode_schedule(mode)
    v, want = LM.oracle_run(O, mode, otab, frames, sched)
    assert len(want) == 3950
    ran = set()
    for kernel, dw in KERNEL_FORMS:
        dev = _device_run(native, O, mode, name, frames, [sched], kernel, dw)
        assert _ran(kernel, dev[4]), (kernel, dw, dev[4])
        ran |= {k for k, n in dev[4].items() if n}
        _compare(native, mode, (mode, name, kernel, dw), dev, v, want)
    assert ran == {"plain", "shared", "team", "workgroup"}
    v4, want4 = LM.oracle_run(O, mode, otab, frames, sched, fourth=True)
    assert (want4[:, 5] != want4[:, 2]).any()                       # fourth offsets that are no copy of the first
    for kernel in FOURTH_KERNELS:
        dev = _device_run(native, O, mode, name, frames, [sched], kernel, fourth=True)
        assert _ran(kernel, dev[4]), (kernel, "fourth", dev[4])
        _compare(native, mode, (mode, name, kernel, "fourth"), dev, v4, want4)
    short = LM.encode_schedule(mode, cap=90)                        # (the oracle's joint step is slow)
    for fourth in (False, True):
        vj, wantj = LM.oracle_run(O, mode, otab, frames, short, fourth=fourth, joint=True)
        for joint, f in JOINT_FORMS:
            if f == fourth:
                dev = _device_run(native, O, mode, name, frames, [short], fourth=fourth, joint=joint)
                assert _ran(False, dev[4]), (joint, fourth, dev[4])           # the joint choice's home is the workgroup kernel
                _compare(native, mode, (mode, name, "joint", joint, fourth), dev, vj, wantj)


@pytest.mark.parametrize("name", LM.MATRICES)
@pytest.mark.parametrize("mode", LM.MODES)
def test_stored_values_at_the_limit_in_every_kernel_form(native, O, mode, name):
    """limit_matrices.store_schedule: bytes that waited take, for want of anything better, extra offsets that mend one dot
    of ten (eighteen) -- with the flat matrix the value a step stores there, pushes into the bag and scores later steps
    against is L * dots - L (tests/test_limit_matrices_host.py).  Every greedy kernel x diff-weight mode and the fourth
    offset against the oracle."""
    otab = oracle_table(O, mode, name)
    frames, sched = LM.store_clip(mode), LM.store_schedule(mode)
    v, want = LM.oracle_run(O, mode, otab, frames, sched)
    for kernel, dw in KERNEL_FORMS:
        dev = _device_run(native, O, mode, name, frames, [sched], kernel, dw)
        assert _ran(kernel, dev[4]), (kernel, dw, dev[4])
        _compare(native, mode, (mode, name, kernel, dw), dev, v, want)
    v4, want4 = LM.oracle_run(O, mode, otab, frames, sched, fourth=True)
    for kernel in FOURTH_KERNELS:
        dev = _device_run(native, O, mode, name, frames, [sched], kernel, fourth=True)
        assert _ran(kernel, dev[4]), (kernel, "fourth", dev[4])
        _compare(native, mode, (mode, name, kernel, "fourth"), dev, v4, want4)


# ---- 5. priorities that cross 16 bits on the device

@pytest.mark.parametrize("name", ["flat", "two_level"])
@pytest.mark.parametrize("mode", LM.MODES)
def test_priorities_cross_16_bits_by_the_prologues_own_additions(native, O, mode, name):
    """Forty rounds of 8 opcodes on a constant white target: a byte that waits gains a diff weight per round, at the limit
    65280 after round 31 and past 65535 -- where the kernels' 16-bit copy hands over to the int32 array -- with round 32.
    The priorities are read after round 31, after round 32 and at the end (two generators on the noise frame later).  Every
    read runs materialise_up_kernel; after round 32, with priorities on both sides of 65535, what was read is also written
    back unchanged, which runs compact_up_kernel, and the encode goes on from the 16-bit copy it rebuilt.  Nothing is
    planted: no priority is set to a value it did not already have."""
    otab = oracle_table(O, mode, name)
    frames = LM.clip(mode)
    parts = LM.crossing_schedule(mode)
    want_ups = []
    sched = [g for p in parts for g in p]
    ends = set(np.cumsum([len(p) for p in parts]) - 1)
    v, want = LM.oracle_run(O, mode, otab, frames, sched,
                            after=lambda v, i: want_ups.append([v.update_priority(b).copy() for b in banks(mode)]) if i in ends else None)
    assert len(want_ups) == 3
    assert all(int(want_ups[0][b].max()) < LM.UP_BIG < int(want_ups[1][b].max()) for b in banks(mode))
    assert all(0 < int(want_ups[1][b][want_ups[1][b] > 0].min()) < LM.UP_BIG for b in banks(mode))     # (both sides of it)
    if name == "flat":
        top = LM.limit(mode) * LM.DOTS[mode]
        assert all(int(want_ups[0][b].max()) == 32 * top and 33 * top == int(want_ups[1][b].max()) for b in banks(mode))
    for kernel in (True, "shared", "team", False):
        dev = _device_run(native, O, mode, name, frames, parts, kernel, write_back=(1,))
        assert _ran(kernel, dev[4]), (kernel, dev[4])
        _compare(native, mode, (mode, name, kernel), dev, v, want, want_ups)
