"""tests/colour_model.py without a device: the model against published data and the recorded tables, the host oracle against
the model on the committed case set (tests/colour_cases.py and the committed rounds of tests/stage_fuzz.py's colour stage) --
where E_HOST, and with it the device's tolerance T = 8 E_HOST, is measured --, the conditions on that case set, and that the
set tells a subtly wrong kernel from a right one."""
import numpy as np
import pytest

import colour_cases as CC
import colour_model as M
import stage_fuzz as F
from test_cie2000_published import SHARMA


@pytest.fixture(scope="module")
def fuzz_cases():
    return [F.draw_colour(F.stage_rng(F.SEED, r, "colour"), r) for r in range(F.ROUNDS["colour"])]


def test_the_model_reproduces_the_published_ciede2000_data():
    got = np.array([float(M.delta_e(tuple(r[0:3]), tuple(r[3:6]))) for r in SHARMA])
    assert np.abs(got - SHARMA[:, 6]).max() < 1e-4, np.abs(got - SHARMA[:, 6])
    back = np.array([float(M.delta_e(tuple(r[3:6]), tuple(r[0:3]))) for r in SHARMA])
    assert np.abs(back - got).max() < 1e-12


@pytest.mark.parametrize("pal", [5, 0])
def test_the_model_reproduces_the_recorded_integer_matrices(O, golden, pal):
    f, i = CC.model_matrix({5: "ntsc", 0: "iigs"}[pal])
    assert np.array_equal(i, golden.g5_tables["dm_i_%d" % pal]) and i.dtype == np.int32
    assert np.array_equal(i, np.floor(f).astype(np.int32))
    assert abs(f[0, 15] - 99.9999849) < 1e-6 and i[0, 15] == 99                # black against white: 1.5e-5 below 100


def test_the_oracle_against_the_model_on_the_committed_cases(O, fuzz_cases, capsys):
    """E_HOST: the largest |oracle - model| over every committed case.  The largest figures are not libm's: a near-grey colour
    has a = 500 (fx - fy) of about 1e-3 with an absolute rounding error of about 5e-14 in double, so its hue is good to 1e-10
    radians or so, and against a saturated colour (sqrt(C1' C2') of about 1) that much reaches delta-H'.  NTSC and IIGS hold
    such pairs; the drawn palettes and the Lab pairs, whose inputs are doubles already, stay below 1.5e-13."""
    worst = {}
    for name, pal in CC.palettes().items():
        f, i = O.cie2000_matrix(pal)
        want_f, want_i = CC.model_matrix(name)
        assert np.array_equal(i, want_i), name
        assert not np.isnan(f).any()
        worst["palette " + name] = float(np.abs(f - want_f).max())
    kinds, lab1, lab2 = CC.pool()
    err = np.abs(O.delta_e_cie2000(lab1, lab2) - CC.model_pool())
    for kind in dict.fromkeys(kinds):
        worst["pairs: " + kind] = float(err[np.array(kinds) == kind].max())
    for r, case in enumerate(fuzz_cases):
        want_f, want_i, want_pairs = F.colour_wants(case)
        f, i = O.cie2000_matrix(case["rgb"])
        assert np.array_equal(i, want_i), r
        worst["stage_fuzz round %d" % r] = float(max(np.abs(f - want_f).max(), np.abs(O.delta_e_cie2000(case["lab1"], case["lab2"]) - want_pairs).max()))
    E = max(worst.values())
    with capsys.disabled():
        print("\nE_host = %.3g (%s); colour_model.E_HOST = %.3g, T = %.3g" % (E, max(worst, key=worst.get), M.E_HOST, M.T))
        print("  " + ", ".join("%s %.2g" % kv for kv in worst.items()))
    assert E < 1e-11
    assert E <= M.E_HOST < 1e-11 and M.T == 8 * M.E_HOST <= 1e-9             # the recorded figure is the measured one, or above it
    assert "E_HOST = %.1e" % M.E_HOST in M.__doc__


def test_the_committed_palettes_keep_off_the_integers():
    pals = CC.palettes()
    assert tuple(pals) == CC.PALETTE_NAMES and set(CC.ingest_model.PALETTES) < set(pals) and len(pals) == 18
    for name in pals:
        f, i = CC.model_matrix(name)
        assert CC.knife_edges_kept(f), name
        same = (pals[name][:, None, :] == pals[name][None, :, :]).all(axis=2)
        assert not f[same].any() and (f[~same] > 1e-3).all(), name             # below 1e-9 means the same colour twice, nothing else
    # what each special palette is there for
    assert pals["dark"].max() <= 23 and {10, 11} <= set(pals["dark"].reshape(-1).tolist())
    lab = [M.lab_double(row) for row in pals["crossover"]]
    assert min(v[0] for v in lab) < 8 < max(v[0] for v in lab)                  # L = 8 is t = 216 / 24389 in Y
    assert (pals["greys"] == pals["greys"][:, :1]).all() and len(np.unique(pals["greys"])) == 16
    chroma = [np.hypot(*M.lab_double(row)[1:]) for row in pals["greys"]]
    assert chroma[0] == 0 and 0 < min(chroma[1:]) and max(chroma) < 0.03        # black has no hue, every other grey a faint one
    assert len(np.unique(pals["corners"], axis=0)) == 8 and len(np.unique(pals["all_equal"], axis=0)) == 1
    # the draws are functions of the seed
    assert np.array_equal(pals["drawn_2"], CC.draw_palette(np.random.default_rng([CC.SEED, 2]), lambda g: g.integers(0, 256, (16, 3)))[0])


def test_the_committed_lab_pairs_keep_off_the_discontinuities():
    kinds, lab1, lab2 = CC.pool()
    assert len(kinds) == CC.POOL == 1000 and lab1.shape == lab2.shape == (1000, 3)
    count = {k: kinds.count(k) for k in dict.fromkeys(kinds)}
    assert count == {"sharma": 34, "axis": 20, "identical": 8, "black and white": 1, "near 180": 36, "near 0": 12, "mean 275": 8,
                     "mean 275, 360 added": 4, "mean L 50": 4, "palette": 256, "uniform": 617}, count
    on_an_edge = []
    for k in range(CC.POOL):
        a, b = tuple(lab1[k].tolist()), tuple(lab2[k].tolist())
        assert CC.pair_allowed(a, b), (k, kinds[k], a, b)
        m = M.margins(a, b)
        if min(m) <= CC.MARGIN:
            on_an_edge.append(k)
            assert kinds[k] in ("sharma", "axis") and (M.on_axis(a) or M.on_axis(b) or M.antipodal(a, b))
        if kinds[k] == "near 180":
            assert 0.5 * CC.EDGE < m[0] < 2 * CC.EDGE and min(m[1:]) > 0.2, (k, m)
        if kinds[k] == "near 0":
            assert 0.5 * CC.EDGE < m[1] < 2 * CC.EDGE and m[0] > 50, (k, m)
        if kinds[k] == "mean L 50":
            assert a[0] + b[0] == 100
    # Sharma's rows 10 and 14 are antipodal, rows 16-24 hold (2.5, 0); three of the four axis families sit on an edge
    assert [k + 1 for k in on_an_edge if kinds[k] == "sharma"] == [10, 14] + list(range(16, 25))
    assert sum(kinds[k] == "axis" for k in on_an_edge) == 15
    # both sides of every edge, and of 275
    near = [k for k in range(CC.POOL) if kinds[k] == "near 180"]
    model = CC.model_pool()
    jumps = np.abs(model[near[0::2]] - model[near[1::2]])
    assert (jumps[np.array(CC.EDGE_CHROMAS * len(CC.EDGE_HUES)) >= 2.5] > 1e-3).all()       # the two sides do differ: the edge is real
    for n in CC.COUNTS:
        idx = CC.subset(n)
        assert len(idx) == len(set(idx.tolist())) == n and idx.max() < CC.POOL
    assert list(CC.subset(64)) != list(CC.subset(65)[:64])


def test_a_draw_that_fails_a_condition_is_drawn_again(monkeypatch):
    """no committed draw came close enough to an edge to be thrown away; with the conditions made 5000 and 10^7 times as
    strict the same code does throw draws away, and what it keeps meets them"""
    monkeypatch.setattr(CC, "KNIFE", 5e-3)
    pal, redraws = CC.draw_palette(np.random.default_rng([CC.SEED, 99]), lambda g: g.integers(0, 256, (16, 3)))
    assert redraws > 0 and CC.knife_edges_kept(CC.matrix_of(pal.tobytes())[0])
    monkeypatch.setattr(CC, "MARGIN", 10.0)
    case = F.draw_colour(F.stage_rng(F.SEED, 4, "colour"), 4)
    assert case["params"]["redraws"] > 0
    assert all(min(M.margins(tuple(a.tolist()), tuple(b.tolist()))) > 10 or M.on_axis(a) or M.on_axis(b) for a, b in zip(case["lab1"], case["lab2"]))


def test_longdouble_gives_the_same_results():
    """the fallback where mpmath does not import: numpy.longdouble against the 50-digit values, well inside T"""
    assert np.finfo(np.longdouble).nmant >= 63                                  # no less than the 80-bit format
    B = M.backend("longdouble")
    worst = 0.0
    for name in ("ntsc", "iigs", "corners", "greys", "dark", "crossover", "drawn_0"):
        f, i = M.matrix(CC.palettes()[name], B)
        want_f, want_i = CC.model_matrix(name)
        assert np.array_equal(i, want_i)
        worst = max(worst, float(np.abs(M.as_float(f) - want_f).max()))
    kinds, lab1, lab2 = CC.pool()
    take = [k for k in range(CC.POOL) if kinds[k] not in ("palette", "uniform")] + list(range(CC.POOL - 100, CC.POOL))
    got = np.array([float(M.delta_e(tuple(lab1[k].tolist()), tuple(lab2[k].tolist()), B)) for k in take])
    worst = max(worst, float(np.abs(got - CC.model_pool()[take]).max()))
    assert worst < M.T / 8, worst


# ---- the committed cases against a kernel that is subtly wrong ------------------------------------------------------------------

class _FloatCubeRoot(M._Mp):
    """pow(v, 1.0 / 3.0) replaced by a single-precision cube root"""

    def power(self, x, y):
        if float(y) == 1.0 / 3.0:
            return self.f(float(np.cbrt(np.float32(float(x)))))
        return super().power(x, y)


def _worst_palette_error(be):
    return max(float(np.abs(M.as_float(M.matrix(CC.palettes()[name], be)[0]) - CC.model_matrix(name)[0]).max()) for name in ("ntsc", "drawn_0"))


def test_the_committed_cases_tell_a_wrong_kernel_from_a_right_one(monkeypatch):
    """Three of the mistakes a kernel could make, made in the model: each moves a committed case by far more than T, so the
    GPU tests would fail on it.  (A fourth, `v < 0.04` for `v <= 0.04045`, can not show through any input: no byte lies
    between 10.2 / 255 and 10.31 / 255.)"""
    assert _worst_palette_error(_FloatCubeRoot()) > 1000 * M.T
    kinds, lab1, lab2 = CC.pool()
    want = CC.model_pool()
    # h' without the 360 added below 0
    monkeypatch.setattr(M, "_hue", lambda B, b, ap: B.f(0.0) if b == 0 and ap == 0 else B.atan2(b, ap) * 180 / B.pi)
    got = np.array([float(M.delta_e(tuple(lab1[k].tolist()), tuple(lab2[k].tolist()))) for k in range(400, 500)])
    assert (np.abs(got - want[400:500]) > 1000 * M.T).sum() > 10
    monkeypatch.undo()
    # a launch of 32 threads a workgroup with the grid of 64: outputs 32 .. n - 1 of a call of n <= 64 are never written, and of
    # the committed counts 63, 64, 65, 128 and 1000 leave pairs unwritten whose delta-E is not 0
    for n in CC.COUNTS[1:]:
        written = 32 * ((n + 63) // 64)
        assert written < n and (want[CC.subset(n)[written:]] > 1).any()
