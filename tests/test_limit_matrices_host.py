"""CPU: do the inputs of tests/test_gpu_limit_matrices.py reach the limit?  The oracle alone, on the matrices, clips and
schedules of tests/limit_matrices.py: the largest table value, diff weight and deltas are the largest the key fields hold,
the encode schedule stores values within one matrix entry of it, and the crossing schedule takes priorities past 16 bits
where the GPU test reads them.  Without these a change to a clip or a seed could leave the GPU tests below the limit
unnoticed."""
import numpy as np
import pytest

import limit_matrices as LM

_otab = {}


def oracle_table(O, mode, name="flat"):
    if (mode, name) not in _otab:
        _otab[(mode, name)] = O.build_table(mode, LM.matrix(mode, name), symmetric=True)
    return _otab[(mode, name)]


def packed(O, mode, f):
    return O.pack(mode, f[0], f[1] if mode == LM.DHGR else None)


def test_matrices_are_what_they_say(O):
    for mode in LM.MODES:
        L = LM.limit(mode)
        assert O.masked_dots(mode) == LM.DOTS[mode] and L == {LM.DHGR: 204, LM.HGR: 113}[mode]
        assert L * LM.DOTS[mode] <= LM.MAX_VALUE < (L + 1) * LM.DOTS[mode]
        for name in LM.MATRICES:
            dm = LM.matrix(mode, name).reshape(16, 16)
            assert dm.min() == 0 and dm.max() == L and not dm.diagonal().any(), (mode, name)
            assert np.array_equal(dm, dm.T) == (name != "lower_wins"), (mode, name)
        flat = LM.matrix(mode, "flat").reshape(16, 16)
        assert (flat[~np.eye(16, dtype=bool)] == L).all()
        two = LM.matrix(mode, "two_level").reshape(16, 16)
        assert two[0, 15] == L and int((np.triu(two, 1) == L).sum()) == 30 and (two[two != L] <= 3).all()
        # ... and is no metric: some dear pair is undercut by a path over two cheap ones
        assert any(two[a, c] + two[c, b] < two[a, b] for a in range(16) for b in range(16) for c in range(16))
        spread = LM.matrix(mode, "spread").reshape(16, 16)
        assert spread[3, 9] == 0 and len(np.unique(spread)) > 40
        low = LM.matrix(mode, "lower_wins").reshape(16, 16)
        assert (low[np.tril_indices(16, -1)] >= L // 2).all() and (low[np.triu_indices(16, 1)] <= 3).all()
        assert (LM.over_limit(mode).max() == L + 1)


def test_clips_are_what_they_say():
    for mode in LM.MODES:
        c = LM.clip(mode)
        assert c.shape == (5, 2, 32, 256) and c.dtype == np.uint8
        assert not c[..., LM.HOLES].any()
        w = LM.WHITE[mode]
        live = ~LM.HOLES
        if mode == LM.DHGR:
            assert c.max() == 0x7f
        else:
            assert not c[:, 1].any() and c.max() == 0xff
        banks = slice(0, 2 if mode == LM.DHGR else 1)
        assert (c[0, banks][..., live] == w).all() and not c[3].any()
        cols = np.arange(256)
        white_cols = ((cols < 64) | ((cols >= 128) & (cols < 192)))
        assert (c[1, banks][..., white_cols & live] == w).all() and not c[1][..., ~white_cols].any()
        assert (c[4, banks][..., (cols % 2 == 0) & live] == w).all() and not c[4][..., cols % 2 == 1].any()
        assert len(np.unique(c[2, 0])) > 100


@pytest.mark.parametrize("mode", LM.MODES)
def test_flat_reaches_the_largest_value_weight_and_deltas(O, mode):
    top = LM.limit(mode) * LM.DOTS[mode]
    table = oracle_table(O, mode)
    assert int(table.max()) == top
    black, white, half = (packed(O, mode, LM.frame(mode, n)) for n in ("black", "white", "half"))
    for ia in ((0, 1) if mode == LM.DHGR else (0,)):
        assert int(O.diff_weights(mode, table, black, white, ia).max()) == top
        dw = O.diff_weights(mode, table, black, half, ia)
        delta = O.compute_delta_page(mode, table, half, 3, LM.WHITE[mode], dw[3], ia)
        assert int(delta.min()) == -top, (mode, ia)
        if mode == LM.DHGR:
            assert int(delta.max()) == top, ia
        else:
            assert int(delta.max()) >= top - 2 * LM.limit(mode)       # (HGR: 1808 of 2034)


def walk(O, mode, table, frames, sched):
    """The oracle over a schedule, watched: the largest priority seen after a segment ("up"), the largest value a step
    left at a SECONDARY offset ("secondary": the entries that are neither zero nor the priority before plus the segment's
    diff weight, video.py:115-116, 166-170), and per segment the length of its sorted list and whether it ran out of work."""
    holes = np.broadcast_to(LM.HOLES, (32, 256))
    seen = {"up": 0, "secondary": 0, "n_secondary_at_limit": 0, "list": [], "out_of_work": [], "ops": 0}
    at_limit = LM.limit(mode) * LM.DOTS[mode] - LM.limit(mode)
    v = O.Video(mode, table, seed_py=5, seed_np=6)
    for (f, ia, restart, k) in sched:
        up = v.update_priority(ia)
        if restart:
            dw = O.diff_weights(mode, table, v.packed, packed(O, mode, frames[f]), ia)
            dw[holes] = 0
            expect = np.where(dw == 0, 0, up) + dw          # video.py:115-116
            v.encode_frame(frames[f, 0], frames[f, 1] if mode == LM.DHGR else None, ia)
        else:
            expect = up.copy()
        seen["list"].append(int((expect != 0).sum()))
        seen["ops"] += len(v.next(k))
        seen["out_of_work"].append(v.out_of_work(ia))
        stored = up[(up != 0) & (up != expect)]
        if stored.size:
            seen["secondary"] = max(seen["secondary"], int(stored.max()))
            seen["n_secondary_at_limit"] += int((stored >= at_limit).sum())
        seen["up"] = max(seen["up"], int(up.max()))
    print(mode, seen)
    return v, seen


@pytest.mark.parametrize("mode", LM.MODES)
def test_encode_schedule_reaches_priorities_at_the_limit_and_the_bag(O, mode):
    """update_priority, read after every segment, holds values within one matrix entry of the limit: the list keys are
    built from them.  The 2200-opcode segment takes its generator through the sorted list (one entry per byte with a
    priority, fewer than the three a step can use up times 2200) and the re-queued bag until it is out of work.
    What a step stores at a secondary offset stays far below on this clip (816 of 2040 in DHGR, 904 of 2034 in HGR):
    that is what store_schedule is for, below."""
    L, dots = LM.limit(mode), LM.DOTS[mode]
    sched = LM.encode_schedule(mode)
    v, seen = walk(O, mode, oracle_table(O, mode), LM.clip(mode), sched)
    assert seen["ops"] == sum(k for (_, _, _, k) in sched)
    assert seen["up"] >= L * dots - L, seen
    i = [k for (_, _, _, k) in sched].index(2200)
    assert 0 < seen["list"][i] < 3 * 2200 and seen["out_of_work"][i], seen


@pytest.mark.parametrize("mode", LM.MODES)
def test_store_schedule_stores_values_at_the_limit(O, mode):
    """Some step of the oracle run stores a value of at least L * dots - L at a secondary offset -- what feeds the pushed
    key's and the step key's value fields; 20 (DHGR) / 16 (HGR) such values are still in place when the run ends.  The screen
    is what the clip says when the waiting starts: the generators before ran out of work."""
    L, dots = LM.limit(mode), LM.DOTS[mode]
    frames, sched = LM.store_clip(mode), LM.store_schedule(mode)
    assert frames.shape == (3, 2, 32, 256) and not frames[..., LM.HOLES].any() and (mode == LM.DHGR or not frames[:, 1].any())
    assert int((frames[1] != frames[0]).sum()) == 32 and int((frames[2] != frames[1]).sum()) == 32 * len(LM.STORE_B)
    v, seen = walk(O, mode, oracle_table(O, mode), frames, sched)
    assert all(seen["out_of_work"][:len(sched) - 2]), seen        # the screen is up before the waiting starts
    assert 32 <= seen["list"][-2] <= 3 * 32, seen                 # (only the As, and in HGR their two neighbours, are pending then)
    assert L * dots - L <= seen["secondary"] < L * dots, seen
    assert seen["n_secondary_at_limit"] >= 1, seen


@pytest.mark.parametrize("name", ["flat", "two_level"])
@pytest.mark.parametrize("mode", LM.MODES)
def test_crossing_schedule_crosses_16_bits_where_it_says(O, mode, name):
    """No priority reaches 65535 before round 32 (with the flat matrix the largest after round 31 is 32 diff weights at the
    limit), some priority of EVERY bank is past 65535 after round 32, and more than 1000 bytes are at the end."""
    top = LM.limit(mode) * LM.DOTS[mode]
    table = oracle_table(O, mode, name)
    frames = LM.clip(mode)
    banks = (0, 1) if mode == LM.DHGR else (0,)
    parts = LM.crossing_schedule(mode)
    assert [len(p) for p in parts] == [32 * len(banks), len(banks), 7 * len(banks) + 2]
    assert parts[2][-2:] == [(2, 0, 1, 300), (2, banks[-1], 1, 300)]
    v = O.Video(mode, table, seed_py=5, seed_np=6)
    peak = []

    def run(part):
        for (f, ia, restart, k) in part:
            v.encode_frame(frames[f, 0], frames[f, 1] if mode == LM.DHGR else None, ia)
            v.next(k)
            peak.append(max(int(v.update_priority(b).max()) for b in banks))

    run(parts[0])
    print(mode, name, "largest priority after round 31:", max(peak))
    assert max(peak) < LM.UP_BIG and (name != "flat" or max(peak) == 32 * top)
    run(parts[1])
    assert all(int(v.update_priority(b).max()) > LM.UP_BIG for b in banks)
    assert name != "flat" or all(int(v.update_priority(b).max()) == 33 * top for b in banks)
    run(parts[2])
    assert sum(int((v.update_priority(b) > LM.UP_BIG).sum()) for b in banks) >= 1000
