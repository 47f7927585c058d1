"""GPU: the 4:2:0 conversion of iiv_resize_frames_yuv420 (csrc/iiv_resize.hip) on all 2^24 (Y, U, V) triples, in each of the
three places it is computed, under the three preset matrices and two matrices at the argument bounds with opposite signs
(tests/yuv_enumeration.py builds the planes; tests/test_yuv_model.py holds, on the model alone, that every triple occurs exactly
once, that every preset puts each of -1, 0, 255 and 256 in front of the clamp in every channel and byte lane, and that the bounds
matrices reach the extremes of the contract).  What a packed clamp would do wrong shows here as a wrong byte.

    B1  yuv_to_rgb_kernel: 16 same-size frames of 1024 x 1024, every triple in one pixel; expected yuv_model.to_rgb of the planes
    B2  the loader of resize_h_kernel<2, YuvRows>: 16384 frames of 1024 constant rows, 4 -> 2 pixels wide, H == h: the horizontal
        pass alone, which a constant row passes unchanged, so every output byte is the loader's conversion
    B3  the loader of resize_h_kernel<1, YuvRows> (w = 4100 > 4096): 4096 constant rows, a seeded sample of the triples next to the
        clamps joined with a uniform one
For B2 and B3 the expected output is yuv_model.to_rgb of one column of the rows, repeated W times: that this is
resize_model.resize(to_rgb(...)) for 4 -> 2 and 4100 -> 2 is test_yuv_model.test_a_constant_row_passes_the_horizontal_pass_unchanged.
The presets run on planar planes, the bounds matrices on interleaved (NV12) ones."""
import numpy as np
import pytest

import yuv_enumeration as E
import yuv_model

pytestmark = pytest.mark.gpu

MATRICES = E.PRESETS + E.BOUNDS_MATRICES
IDS = list(E.PRESETS) + ["bounds_a", "bounds_b"]
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _device_planes(y, u, v, matrix):
    """the planes on the device: planar for a preset, interleaved chroma for a bounds matrix"""
    import torch
    dy = torch.from_numpy(np.array(y)).cuda()                         # (copies: the cached planes are read-only)
    if isinstance(matrix, str):
        return dy, torch.from_numpy(np.array(u)).cuda(), torch.from_numpy(np.array(v)).cuda()
    uv = torch.from_numpy(np.stack([u, v], axis=-1)).cuda()
    return dy, uv[..., 0], uv[..., 1]


def _compare(got, exp, y, u, v):
    """got CUDA (n, h, W, 3); exp numpy (n, h, 1 or W, 3), compared on the device; a difference names its triples"""
    import torch
    e = torch.from_numpy(np.ascontiguousarray(exp)).cuda()
    bad = (got != e).any(dim=-1)                                      # (broadcasts a one-column expectation over W)
    n_bad = int(bad.sum())
    if n_bad:
        at = torch.nonzero(bad)[:5].cpu().numpy()
        h, w = y.shape[-2:]
        lines = []
        for f, r, c in at:
            src = c * w // got.shape[2] if w != got.shape[2] else c
            lines.append("frame %d row %d column %d: (Y, U, V) = (%d, %d, %d), got %s, model %s"
                         % (f, r, c, y[f, r, src], u[f, r >> 1, src >> 1], v[f, r >> 1, src >> 1], got[f, r, c].cpu().numpy(),
                            exp[f, r, min(c, exp.shape[2] - 1)]))
        raise AssertionError("%d of %d pixels differ from the model:\n%s" % (n_bad, bad.numel(), "\n".join(lines)))


@pytest.mark.parametrize("matrix", MATRICES, ids=IDS)
def test_same_size_frames_over_all_triples(native, matrix):
    """B1: the conversion kernel's own bytes (the same-size resize behind it is a copy)"""
    import torch
    y, u, v = _cached("b1", E.b1_planes)
    n, h, w = E.B1_SHAPE
    exp = yuv_model.to_rgb(y, u, v, matrix)
    got = native.resize_frames_yuv420(*_device_planes(y, u, v, matrix), (h, w), matrix=matrix)
    assert tuple(got.shape) == (n, h, w, 3)
    _compare(got, exp, y, u, v)
    del got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("matrix", MATRICES, ids=IDS)
def test_two_row_loader_over_all_triples(native, matrix):
    """B2: resize_h_kernel<2, YuvRows>, every triple a constant row"""
    import torch
    cy, cu, cv = _cached("b2", E.b2_columns)
    n, h = E.B2_SHAPE
    w, W = 4, 2
    exp = yuv_model.to_rgb(cy, cu, cv, matrix)                        # (n, h, 1, 3)
    y, u, v = _cached("b2 wide", lambda: E.widen(cy, cu, cv, w))
    got = native.resize_frames_yuv420(*_device_planes(y, u, v, matrix), (h, W), matrix=matrix)
    assert tuple(got.shape) == (n, h, W, 3)
    _compare(got, exp, y, u, v)
    del got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("matrix", MATRICES, ids=IDS)
def test_one_row_loader_on_the_boundary_sample(native, matrix):
    """B3: resize_h_kernel<1, YuvRows>"""
    cy, cu, cv = E.b3_columns(matrix)
    w, W = E.B3_WIDTH, 2
    assert ((w + 3) & ~3) > 4096 and cy.shape[0] * cy.shape[1] == 4096
    exp = yuv_model.to_rgb(cy, cu, cv, matrix)
    y, u, v = E.widen(cy, cu, cv, w)
    got = native.resize_frames_yuv420(*_device_planes(y, u, v, matrix), (2, W), matrix=matrix)
    assert tuple(got.shape) == (E.B3_FRAMES, 2, W, 3)
    _compare(got, exp, y, u, v)
