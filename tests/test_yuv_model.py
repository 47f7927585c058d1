"""CPU: tests/yuv_model.py -- the 4:2:0 YCbCr -> RGB contract of include/iivision.h f11 -- against known points, against the
real-valued matrices its presets round, and for the chroma sample every pixel takes; and the preset table of the package
against the contract's bounds."""
import numpy as np
import pytest

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
