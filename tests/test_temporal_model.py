"""CPU: section f14 of include/iivision.h as tests/temporal_model.py restates it, held to the properties the section states, and the
entry point's host side: the symbol, its place in the binding, and every refusal, which the library decides before it touches a
device.  The full-hold clip is shown to bite: without the hold its memory maps differ from frame to frame."""
import ctypes as C

import numpy as np
import pytest

import ingest_model
import temporal_cases as TC
import temporal_model as M


def _noise(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def test_identity_at_zero_zero():
    x = _noise(1, (6, 40, 3))
    out, state, counts = M.hold(x, 0, 0)
    assert np.array_equal(out, x) and np.array_equal(state, x[-1])
    out2, _, _ = M.hold(x, 0, 0, state=_noise(2, (40, 3)))
    assert np.array_equal(out2, x)
    # a pixel that repeats is counted held, one that moves passed, none blended
    assert (counts[:, 1] == 0).all() and counts[0, 2] == 40
    still = np.repeat(x[:1], 3, axis=0)
    assert [tuple(c) for c in M.hold(still, 0, 0)[2]] == [(0, 0, 40), (40, 0, 0), (40, 0, 0)]


@pytest.mark.parametrize("lo,hi", TC.PAIRS + ((0, 254), (1, 255), (100, 101)))
def test_weights_are_monotone_with_their_end_values(lo, hi):
    w = M.weights(lo, hi)
    assert w.shape == (256,) and (np.diff(w) >= 0).all()
    assert (w[:lo + 1] == 0).all() and (w[hi + 1:] == 256).all()
    between = w[lo + 1:hi + 1]
    assert len(between) == hi - lo and (between >= 1).all() and (between <= 255).all()
    for d in range(lo + 1, hi + 1):
        assert w[d] == (256 * (d - lo)) // (hi - lo + 1)


@pytest.mark.parametrize("lo,hi", TC.PAIRS)
@pytest.mark.parametrize("kind", TC.KINDS)
def test_counts_sum_to_the_pixels(kind, lo, hi):
    _, counts = TC.want(kind, 260, (lo, hi))
    assert counts.shape == (TC.CLIPS, TC.FRAMES, 3) and (counts.astype(np.int64).sum(axis=2) == 260).all()
    assert (counts[:, 0] == (0, 0, 260)).all()          # a first frame passes whole
    if lo == hi:
        assert (counts[:, :, 1] == 0).all()             # nothing lies between lo and hi


@pytest.mark.parametrize("lo,hi", TC.PAIRS)
def test_a_split_with_the_state_carried_equals_one_call(lo, hi):
    x = TC.clip("near", 252)[0]
    whole, state, counts = M.hold(x, lo, hi)
    for cut in (1, 5, TC.FRAMES - 1):
        a, sa, ca = M.hold(x[:cut], lo, hi)
        b, sb, cb = M.hold(x[cut:], lo, hi, state=sa)
        assert np.array_equal(np.concatenate([a, b]), whole) and np.array_equal(sb, state)
        assert np.array_equal(np.concatenate([ca, cb]), counts)
        assert np.array_equal(sa, whole[cut - 1])


def test_a_ramp_moves_on_every_fifth_frame():
    """+1 a frame under lo = hi = 4: the held value stays for four frames and jumps to the source on the fifth"""
    x = np.clip(np.arange(23)[:, None, None] + np.array([[[10, 100, 200]]]), 0, 255).astype(np.uint8)
    out, _, counts = M.hold(x, 4, 4)
    moved = [t for t in range(1, 23) if not np.array_equal(out[t], out[t - 1])]
    assert moved == [5, 10, 15, 20]
    for t in range(23):
        assert np.array_equal(out[t], x[t - t % 5])
    assert [int(c[2]) for c in counts] == [1 if t % 5 == 0 else 0 for t in range(23)]


def test_the_extreme_product_stays_in_range():
    """0 <-> 255 under (0, 255): w = 255, (x - h) * w + 128 = +-65025 + 128; the shift floors towards minus infinity"""
    x = np.array([[[0, 255, 0]], [[255, 0, 255]], [[0, 255, 0]]], np.uint8)
    out, _, _ = M.hold(x, 0, 255)
    assert M.weights(0, 255)[255] == 255
    assert out[1].tolist() == [[254, 1, 254]]            # 0 + (65153 >> 8) = 254; 255 + (-64897 >> 8) = 255 - 254
    assert out[2].tolist() == [[2, 253, 2]]              # d = 254: w = 254; 254 + ((-64516 + 128) >> 8) = 254 - 252; 1 + (64644 >> 8)


def test_the_gpu_grid_meets_every_branch():
    """the inputs of tests/test_gpu_temporal.py, on the model: they hold, blend and pass pixels, and the flip reaches the extreme
    product"""
    for pair in ((4, 4), (3, 12), (16, 64)):
        assert TC.want("near", 1028, pair)[1][:, 1:, 0].sum() > 0                  # held
    assert TC.want("near", 1028, (4, 4))[1][:, 1:, 2].sum() > 0                    # passed, beside held
    assert TC.want("near", 1028, (3, 12))[1][:, 1:, 1].sum() > 0                   # blended, beside held
    assert TC.want("noise", 1028, (16, 64))[1][:, 1:].sum(axis=(0, 1)).min() > 0    # all three
    assert TC.want("ramp", 1028, (4, 4))[1][:, 1:, [0, 2]].sum(axis=(0, 1)).min() > 0
    out, _ = TC.want("flip", 256, (0, 255))
    assert {254, 1} <= set(np.unique(out[:, 1]).tolist())


def test_full_hold_repeats_frame_zero_and_the_input_bites():
    x = TC.still_clip()
    a = TC.HOLD_AMPLITUDE
    assert TC.HOLD_PAIR[0] >= 2 * a and x.shape == (TC.HOLD_FRAMES, 192, 280, 3)
    assert int(np.abs(x.astype(np.int64) - x[:1]).max()) == 2 * a           # the bound is met, not just respected
    out, state, counts = M.hold(x, *TC.HOLD_PAIR)
    assert (out == x[:1]).all() and np.array_equal(state, x[0])
    assert (counts[1:] == (192 * 280, 0, 0)).all()
    # without the hold the ordered dither's memory maps differ from frame to frame; behind it they do not
    pal = ingest_model.PALETTES["corners"]
    main, aux = ingest_model.frames_to_memory_maps(ingest_model.DHGR, pal, x[:3], 32)
    assert (main[1] != main[0]).any() and (main[2] != main[1]).any() and (aux[1] != aux[0]).any()
    main_h, aux_h = ingest_model.frames_to_memory_maps(ingest_model.DHGR, pal, out[:3], 32)
    assert (main_h == main_h[:1]).all() and (aux_h == aux_h[:1]).all() and np.array_equal(main_h[0], main[0])


# ---- the entry point's host side -----------------------------------------------------------------------------------------------------

def test_the_entry_point_is_declared_and_exported(native):
    assert "iiv_temporal_hold" in native.SYMBOLS
    f = native.lib().iiv_temporal_hold
    assert f.restype is C.c_int and len(f.argtypes) == 16 and f.argtypes[2] is C.c_long and f.argtypes[4] is C.c_size_t


def test_refusals_need_no_device(native):
    """every refusal of the header, with pointers that are never followed: the library decides before anything is launched"""
    L = native.lib()
    base = 1 << 20

    def call(c=2, n=3, pixels=8, src=base, scs=96, sfs=24, out=base + 4096, ocs=96, ofs=24, state=base + 8192, ss=24, first=1,
             lo=3, hi=12, counts=base + 12288):
        return L.iiv_temporal_hold(c, n, pixels, C.c_void_p(src), scs, sfs, C.c_void_p(out), ocs, ofs, C.c_void_p(state), ss, first,
                                   lo, hi, C.c_void_p(counts), None)
    refused = [call(c=-1), call(n=-1), call(pixels=0), call(pixels=-4), call(pixels=6), call(pixels=9),
               call(src=base + 2), call(out=base + 4097), call(state=base + 8194), call(counts=base + 12290),
               call(scs=98), call(sfs=26), call(ocs=94), call(ofs=30), call(ss=26),
               call(sfs=20), call(ofs=20), call(ss=20),
               call(lo=-1), call(hi=256), call(lo=13), call(lo=256, hi=256), call(lo=-2, hi=-1),
               call(src=0), call(out=0), call(state=0)]
    assert refused == [native.ERR_INVALID] * len(refused)
    assert b"iiv_temporal_hold" in L.iiv_last_error()
    # no work: success, nothing touched (the pointers are not even looked at)
    assert call(c=0) == 0 and call(n=0) == 0 and call(c=0, src=0, out=0, state=0, counts=0) == 0
    for pair in ((0, 0), (3, 2), (0, 256), (-1, 4), (1.5, 3), "ab", (1, 2, 3), None):
        if pair == (0, 0):
            assert native.temporal_pair(pair) == (0, 0)
        else:
            with pytest.raises(ValueError):
                native.temporal_pair(pair)
