"""CPU: tests/yuv_model.py -- the 4:2:0 YCbCr -> RGB contract of include/iivision.h f11 -- against known points, against the
real-valued matrices its presets round, and for the chroma sample every pixel takes; and the preset table of the package
against the contract's bounds; then the conditions the exhaustive GPU tests rest on (tests/yuv_enumeration.py): every triple
exactly once, the clamps' edges in every channel and byte lane, the extremes under the bounds matrices, and the constant-row
identity of the horizontal pass at the size pairs those tests use."""
import numpy as np
import pytest

import resize_model
import yuv_enumeration as E
import yuv_model as M


def _one(y, u, v, matrix):
    return tuple(int(c) for c in M.to_rgb(np.full((1, 1), y, np.uint8), np.full((1, 1), u, np.uint8), np.full((1, 1), v, np.uint8),
                                          matrix)[0, 0])


def test_known_points_bt601():
    assert _one(16, 128, 128, "bt601") == (0, 0, 0)
    assert _one(235, 128, 128, "bt601") == (255, 255, 255)
    # Y = 0 is below black: c = -16, ky c = -4768, and what leaves 0..255 is clamped, channel by channel
    assert _one(0, 128, 128, "bt601") == (0, 0, 0)        # (-4768 + 128) >> 8 = -19
    assert _one(0, 0, 0, "bt601") == (0, 135, 0)          # R -57, B -69; G = (-4768 + 12800 + 26624 + 128) >> 8
    assert _one(0, 255, 255, "bt601") == (184, 0, 237)    # G = (-4768 - 12700 - 26416 + 128) >> 8 = -171
    # (255, 255, 255): R = (239 * 298 + 127 * 409 + 128) >> 8 = 481, B = 534: clamped; G = (71222 - 12700 - 26416 + 128) >> 8 = 125
    assert _one(255, 255, 255, "bt601") == (255, 125, 255)


# Kr, Kb of the three standards; limited range scales luma by 255 / 219 and chroma by 255 / 224, full range by 1
STANDARDS = {"bt601": (0.299, 0.114, 16, 255.0 / 219.0, 255.0 / 224.0), "bt709": (0.2126, 0.0722, 16, 255.0 / 219.0, 255.0 / 224.0),
             "jpeg": (0.299, 0.114, 0, 1.0, 1.0)}


def _real(y, u, v, name):
    kr, kb, y_off, sy, sc = STANDARDS[name]
    kg = 1.0 - kr - kb
    c, d, e = sy * (y - y_off), sc * (u - 128.0), sc * (v - 128.0)
    r = c + 2.0 * (1.0 - kr) * e
    g = c - 2.0 * (1.0 - kb) * kb / kg * d - 2.0 * (1.0 - kr) * kr / kg * e
    b = c + 2.0 * (1.0 - kb) * d
    return np.clip(np.stack([r, g, b], -1), 0.0, 255.0)


@pytest.mark.parametrize("name", sorted(M.MATRICES))
def test_presets_are_within_one_of_the_real_matrix(name):
    lat = np.arange(0, 256, 17)                       # 0, 17, ..., 255
    y, u, v = (a.reshape(-1).astype(np.uint8) for a in np.meshgrid(lat, lat, lat, indexing="ij"))
    grey = np.arange(256, dtype=np.uint8)
    y, u, v = np.concatenate([y, grey]), np.concatenate([u, np.full(256, 128, np.uint8)]), np.concatenate([v, np.full(256, 128, np.uint8)])
    # (one 1 x 1 frame per point: in a row of pixels, pixel x would take sample x >> 1)
    got = np.stack([M.to_rgb(y[i:i + 1, None], u[i:i + 1, None], v[i:i + 1, None], name)[0, 0] for i in range(len(y))]).astype(np.float64)
    exp = _real(y.astype(np.float64), u.astype(np.float64), v.astype(np.float64), name)
    assert np.abs(got - exp).max() <= 1.0, np.abs(got - exp).max()


@pytest.mark.parametrize("h,w", [(5, 7), (1, 1), (2, 3), (4, 4), (3, 8)])
def test_every_pixel_takes_the_sample_at_half_its_coordinates(h, w):
    ch, cw = (h + 1) // 2, (w + 1) // 2
    rng = np.random.RandomState(h * 16 + w)
    y = rng.randint(0, 256, (h, w)).astype(np.uint8)
    u = (np.arange(ch * cw).reshape(ch, cw) * 7 + 3).astype(np.uint8)         # every sample its own value
    v = (250 - np.arange(ch * cw).reshape(ch, cw) * 5).astype(np.uint8)
    got = M.to_rgb(y, u, v, "bt709")
    assert got.shape == (h, w, 3)
    for yy in range(h):
        for xx in range(w):                                                       # up to the last row and column of an odd frame
            assert tuple(got[yy, xx]) == _one(y[yy, xx], u[yy >> 1, xx >> 1], v[yy >> 1, xx >> 1], "bt709"), (yy, xx)
    # frames are independent
    assert np.array_equal(M.to_rgb(np.stack([y, y[::-1]]), np.stack([u, u]), np.stack([v, v]), "bt709")[0], got)


def test_preset_table_is_the_contracts_and_within_its_bounds():
    import frame_grabber
    import _iiv_native as native
    assert frame_grabber.YUV_MATRICES == M.MATRICES and frame_grabber.YUV_MATRICES is native.YUV_MATRICES
    for name, m in frame_grabber.YUV_MATRICES.items():
        assert len(m) == 6 and 0 <= m[0] <= 255 and all(abs(k) <= 1023 for k in m[1:]), name
        assert native.yuv_matrix(name).tolist() == list(m) and native.yuv_matrix(m).dtype == np.int32
    # the bounds keep every sum inside int32 with room to spare: three products of at most 1023 * 255, and the rounding
    assert 3 * 1023 * 255 + 128 < 1 << 20
    with pytest.raises(ValueError):
        native.yuv_matrix("bt2020")
    with pytest.raises(ValueError):
        native.yuv_matrix((16, 298, 409))


# ---- the conditions tests/test_gpu_yuv_exhaustive.py rests on, asserted on the model alone (tests/yuv_enumeration.py) ----------

def test_shifted_sums_are_the_models_before_its_clamp():
    y, u, v = M.random_planes(1, 64, 64, seed=9)
    for matrix in E.PRESETS + E.BOUNDS_MATRICES:
        s = E.shifted_sums(y, E.upsampled(u, 64, 64), E.upsampled(v, 64, 64), matrix)
        assert np.array_equal(np.clip(s, 0, 255).astype(np.uint8), M.to_rgb(y, u, v, matrix)), matrix


def test_the_enumerations_hold_each_triple_exactly_once():
    y, u, v = E.b1_planes()
    assert y.shape == E.B1_SHAPE and u.shape == v.shape == (16, 512, 512)
    assert (np.bincount(E.triple_keys(y, u, v).reshape(-1), minlength=1 << 24) == 1).all()
    y, u, v = E.b2_columns()
    assert y.shape == E.B2_SHAPE + (1,) and u.shape == v.shape == (16384, 512, 1)
    assert (np.bincount(E.triple_keys(y, u, v).reshape(-1), minlength=1 << 24) == 1).all()
    wy, wu, wv = E.widen(y[:2, :6], u[:2, :3], v[:2, :3], 4)
    assert wy.shape == (2, 6, 4) and wu.shape == (2, 3, 2) and (wy == y[:2, :6]).all() and (wu == u[:2, :3]).all() and (wv == v[:2, :3]).all()
    y, u, v = E.all_triples()
    assert len(np.unique((y.astype(np.int64) << 16) | (u.astype(np.int64) << 8) | v)) == 1 << 24


@pytest.mark.parametrize("matrix", E.PRESETS)
def test_every_preset_meets_both_clamps_edges_in_every_channel_and_byte_lane(matrix):
    """sum >> 8 takes each of -1, 0, 255 and 256 in every channel, in every lane x mod 4 of the same-size frames (a thread of
    yuv_to_rgb_kernel converts pixels 4 g .. 4 g + 3 and packs their bytes into three dwords)"""
    y, u, v = E.b1_planes()
    n, h, w = E.B1_SHAPE
    s = E.shifted_sums(y, E.upsampled(u, h, w), E.upsampled(v, h, w), matrix)
    total = {}
    for value in E.EDGE_VALUES:
        hit = s == value
        for lane in range(4):
            for c in range(3):
                assert hit[:, :, lane::4, c].any(), (matrix, value, lane, c)
        total[value] = int(hit.sum())
    assert all(90000 <= t <= 100000 for t in total.values()), total       # 94 000 to 99 000 triples a value, over the channels
    out = ((s < 0) | (s > 255)).any(axis=-1).mean()
    assert out > 0.3, out                                   # the triples that leave 0..255 in some channel: no corner of the domain


@pytest.mark.parametrize("matrix,extremes", list(zip(E.BOUNDS_MATRICES, E.BOUNDS_EXTREMES)))
def test_the_bounds_matrices_reach_the_extremes_of_the_contract(matrix, extremes):
    assert matrix[0] in (0, 255) and all(abs(k) == 1023 for k in matrix[1:])
    s = E.shifted_sums(*E.all_triples(), matrix)
    assert (int(s.min()), int(s.max())) == extremes
    assert abs(int(s.min())) << 8 < 1 << 20 and int(s.max()) << 8 < 1 << 20       # the header's bound on a sum
    for c in range(3):
        assert (s[:, c] < 0).any() and (s[:, c] > 255).any() and ((s[:, c] >= 0) & (s[:, c] <= 255)).any(), c     # both clamps, and neither
        assert not np.isin(s[:, c], (-1, 255)).any()          # 1023 k + 128 never lands in [-256, -1] or [65280, 65535]: not asked for
    edge = E.boundary_triples(matrix)
    assert len(edge) > 1024 and np.isin(E.shifted_sums(edge[:, 0], edge[:, 1], edge[:, 2], matrix), (0, 256)).any(axis=1).all()


@pytest.mark.parametrize("w,W", [(4, 2), (E.B3_WIDTH, 2)])
def test_a_constant_row_passes_the_horizontal_pass_unchanged(w, W):
    """the identity the exhaustive GPU tests use for their expected output: to_rgb of one column, repeated W times, is
    resize_model.resize(to_rgb(the constant rows)) -- for every byte value, at the size pairs those tests use"""
    rows = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None], (256, w, 3))[None]
    assert np.array_equal(resize_model.resize(rows, (256, W)), np.broadcast_to(rows[:, :, :1], (1, 256, W, 3)))


@pytest.mark.parametrize("matrix", E.PRESETS + E.BOUNDS_MATRICES)
def test_the_one_row_sample_holds_boundary_and_uniform_triples(matrix):
    y, u, v = E.b3_columns(matrix)
    assert y.shape == (E.B3_FRAMES, 2, 1) and u.shape == v.shape == (E.B3_FRAMES, 1, 1)
    half = E.B3_FRAMES // 2
    s = E.shifted_sums(y[:half, 0, 0], u[:half, 0, 0], v[:half, 0, 0], matrix)
    if isinstance(matrix, str):
        assert np.isin(s, E.EDGE_VALUES).any(axis=1).all()
        for c in range(3):
            assert set(E.EDGE_VALUES) <= set(np.unique(s[:, c]).tolist()), (matrix, c)
    else:
        assert np.isin(s, (0, 256)).any(axis=1).all() and (s < 0).any() and (s > 255).any()
    assert len(np.unique(E.triple_keys(y, u, v))) > 0.99 * 2 * E.B3_FRAMES
    y2, u2, v2 = E.b3_columns(matrix)
    assert np.array_equal(y, y2) and np.array_equal(u, u2) and np.array_equal(v, v2)      # seeded
