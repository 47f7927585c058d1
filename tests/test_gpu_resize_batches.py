"""GPU: csrc/iiv_resize.hip past its first piece.  iiv_resize_frames cuts a call into chunks of frames (two passes: the
intermediate of one chunk is kChunkMidBytes, at most 65536 frames), slices (one pass: 65536 frames) and launches (at most
2^32 - 1 work-items each).  Every case here crosses at least one of those boundaries, and every frame of it is compared
with the tests' model (tests/resize_model.py).

The batches are periodic: frame i is base[i % P] with P = 7, prime to every piece size below, so the model runs P times
and a piece that reads or writes the wrong frames lands on different content."""
import numpy as np
import pytest

import resize_model as M

pytestmark = pytest.mark.gpu

P = 7
CHUNK_MID_BYTES = 32 << 20     # iiv_resize.hip:34 kChunkMidBytes: the two-pass intermediate of one chunk
MAX_CHUNK_FRAMES = 65536       # iiv_resize.hip, iiv_resize_frames: the chunk cap, and the one-pass slice
MAX_LAUNCH_ITEMS = (1 << 32) - 1   # work-items in one launch dimension


def chunk_frames(h, w, H, W):
    """frames per chunk of a two-pass resize (iiv_resize_frames: mid_rs, mid_fs, chunk)"""
    v_first = M.vertical_first(h, w)
    mid_rs = ((3 * w if v_first else 3 * W) + 3) & ~3
    mid_fs = (H if v_first else h) * mid_rs
    return max(1, min(CHUNK_MID_BYTES // mid_fs, MAX_CHUNK_FRAMES))


def _base(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(P, h, w, 3)).astype(np.uint8)


def _periodic(base_dev, n):
    """CUDA (n, h, w, 3): frame i = base[i % P]"""
    import torch
    return base_dev[torch.arange(n, device=base_dev.device) % P]


def _check_periodic(out, exp):
    """out: CUDA (n, H, W, 3); exp: numpy (P, H, W, 3), the model of base -- every frame i equals exp[i % P]"""
    import torch
    n = out.shape[0]
    e = torch.from_numpy(np.ascontiguousarray(exp)).to(out.device)
    bad = torch.zeros(n, dtype=torch.bool, device=out.device)
    for r in range(P):
        bad[r::P] = (out[r::P] != e[r]).flatten(1).any(1)
    idx = torch.nonzero(bad).flatten().cpu().numpy()
    assert len(idx) == 0, "%d of %d frames differ from the model, the first at %s" % (len(idx), n, idx[:10])


def _run(native, h, w, H, W, n, seed):
    import torch
    base = _base(h, w, seed)
    src = _periodic(torch.from_numpy(base).cuda(), n)
    out = native.resize_frames(src, (H, W))
    del src
    _check_periodic(out, M.resize(base, (H, W)))
    del out
    torch.cuda.empty_cache()


def test_two_passes_horizontal_first_across_chunks(native):
    """640x480 -> 280x192: the (480, 280) intermediate is 403200 bytes a frame, 83 frames a chunk; chunks of 83, 83, 5"""
    h, w, H, W = 480, 640, 192, 280
    assert not M.vertical_first(h, w) and chunk_frames(h, w, H, W) == 83
    _run(native, h, w, H, W, 2 * 83 + 5, 1)


def test_two_passes_vertical_first_across_chunks(native):
    """300x2 -> 192x16 (h > 100 w): the (192, 2) intermediate is 1536 bytes a frame, 21845 frames a chunk"""
    h, w, H, W = 300, 2, 192, 16
    assert M.vertical_first(h, w) and chunk_frames(h, w, H, W) == 21845
    _run(native, h, w, H, W, 2 * 21845 + 7, 2)


def test_two_passes_chunk_cap(native):
    """4x4 -> 3x3: the intermediate is 48 bytes a frame, so the 65536-frame cap makes the chunks"""
    h, w, H, W = 4, 4, 3, 3
    assert chunk_frames(h, w, H, W) == MAX_CHUNK_FRAMES
    _run(native, h, w, H, W, MAX_CHUNK_FRAMES + 7, 3)


@pytest.mark.parametrize("h,w,H,W", [(4, 8, 4, 5), (8, 4, 5, 4)])
def test_one_pass_slices(native, h, w, H, W):
    """one pass (horizontal only, vertical only) goes straight to the output in slices of 65536 frames"""
    assert (H == h) != (W == w)
    _run(native, h, w, H, W, MAX_CHUNK_FRAMES + 9, 4 + h)


def test_crop_view_across_chunks(native):
    """a 480x640 crop of 500x700 frames: the frame stride (1050000) is not h * 3w, the row stride not 3w, and the first
    byte not 4-byte aligned; chunks of 83, 83, 5"""
    import torch
    n, (H, W) = 2 * 83 + 5, (192, 280)
    base = _base(500, 700, 5)
    big = _periodic(torch.from_numpy(base).cuda(), n)
    view = big[:, 10:490, 30:670]
    assert view.stride(0) != 480 * 640 * 3 and view.stride(1) != 640 * 3 and view.storage_offset() % 4 != 0
    assert chunk_frames(480, 640, H, W) == 83
    out = native.resize_frames(view, (H, W))
    del big, view
    _check_periodic(out, M.resize(base[:, 10:490, 30:670], (H, W)))
    del out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("h,w", [(1, 1), (1, 2)])
def test_grid_limit(native, h, w):
    """-> 1024x1: the vertical pass is 1024 workgroups of 256 work-items a frame, so 20000 frames in one launch would be
    5.2e9 work-items.  (1, 1): one vertical pass in one 65536-frame slice; (1, 2): a horizontal pass then the vertical
    one, in one chunk (the intermediate is 4 bytes a frame)."""
    n, H, W = 20000, 1024, 1
    assert n * H * 256 > MAX_LAUNCH_ITEMS
    if w != W:
        assert not M.vertical_first(h, w) and chunk_frames(h, w, H, W) == MAX_CHUNK_FRAMES
    _run(native, h, w, H, W, n, 6 + w)
