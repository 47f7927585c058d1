"""GPU: iiv_resize_frames_yuv420 (csrc/iiv_resize.hip) past the first piece of each of its host loops, as
tests/test_gpu_resize_batches.py does for iiv_resize_frames.  A call is cut into frames in three places -- the entry point's
conversion chunks, and the slices and chunks of resize_rows, the driver it shares with iiv_resize_frames -- and each moves three
plane pointers with from_frame -- luma by y_frame_stride, both chroma planes by c_frame_stride:

    unfused    (W == w, or H != h and h > 100 w) yuv_to_rgb_kernel converts chunks of 32 MiB // (h * 3 * w_pad) frames, no cap,
               into scratch and hands each chunk to resize_rows<RgbRows>, iiv_resize_frames' driver (which slices and chunks it
               again on its own)
    fused      (both axes change, horizontal first) resize_h_kernel<R, YuvRows> fills the (h, W) intermediate in chunks of
               min(32 MiB // (h * mid_rs), 65536) frames
    one pass   (H == h) resize_h_kernel<R, YuvRows> straight to the output in slices of 65536 frames

Frame i of every plane is base[i % 7], gathered on the device; the model -- resize_model.resize(yuv_model.to_rgb(base)) -- runs
on the seven, and every frame of the batch is compared on the device.  Every piece length is prime to 7, so a piece that reads or
writes the wrong frames, or reads one plane's frames at another plane's stride, lands on other content.  Two layouts a case: planar
with padding rows behind every plane's frame (c_frame_stride is neither y_frame_stride / 4 nor ch * cw), and interleaved NV12 cut
out of a larger allocation (chroma pixel stride 2); everything outside the planes holds a fill byte.

launch_h<YuvRows>'s own frames_per_launch step is not reached here, and cannot be at a size a test can hold.  A launch takes up to
2^32 - 1 work-items; launch_h<YuvRows> is handed fn <= 65536 frames of bpf = ceil(h / R) workgroups of T = W rounded up to 64
threads, so the step acts only where fn * bpf * T >= 2^32.
    fused     fn <= 32 MiB / (h * mid_rs) with mid_rs >= max(3 W, 4) and bpf <= h: fn * bpf * T <= 32 MiB * T / mid_rs, which is
              2^25 * 64 / 4 = 2^29 up to W = 64 and less than 2^25 * (W + 63) / (3 W) < 2^25 beyond it.  Never.
    one pass  H == h <= 1024, so bpf <= 1024, and 65536 * bpf * T >= 2^32 needs bpf * T >= 65536.  With two rows a workgroup
              (w <= 4096) bpf <= 512, so T >= 128, W >= 65, and the output is 65536 * h * 3 W bytes with h >= 2 bpf - 1: the
              least is 65536 * 1023 * 195 = 13 GB at W = 65 (24 GB at T = 1024, W = 961).  With one row a workgroup (w > 4096)
              bpf = h = 1024 and T = 64 do, but the luma plane alone is 65536 * 1024 * 4097 bytes = 275 GB.
The launch loop is the one the RGB rows go through (test_gpu_resize_batches.test_grid_limit crosses the step through the
vertical pass)."""
import numpy as np
import pytest

import resize_model
import yuv_model
from test_gpu_resize_batches import CHUNK_MID_BYTES, MAX_CHUNK_FRAMES, P, _check_periodic

pytestmark = pytest.mark.gpu

FILL = 0xC7


def path(h, w, H, W):
    """which of the three ways through iiv_resize_frames_yuv420 a shape takes (iiv_resize.hip: horizontal_first, resize_rows)"""
    resize_w, resize_h = W != w, H != h
    if not resize_w or (resize_h and h > 100 * w):
        return "unfused"
    return "fused" if resize_h else "one pass"


def unfused_chunk(h, w):
    """frames per conversion chunk (rgb_rs, rgb_fs, chunk): no 65536 cap"""
    return max(1, CHUNK_MID_BYTES // (h * 3 * ((w + 3) & ~3)))


def fused_chunk(h, W):
    """frames per chunk of the fused two-pass path (mid_rs, mid_fs, chunk)"""
    return max(1, min(CHUNK_MID_BYTES // (h * ((3 * W + 3) & ~3)), MAX_CHUNK_FRAMES))


# (id, h, w, H, W, the path, the piece length the case relies on, frames)
CASES = [("fused_chunk_by_bytes", 48, 64, 24, 40, "fused", 5825, 2 * 5825 + 5),
         ("fused_chunk_cap", 8, 33, 3, 7, "fused", 65536, 65536 + 7),
         ("one_pass_slice", 6, 10, 6, 4, "one pass", 65536, 65536 + 9),
         ("unfused_same_size", 5, 5, 5, 5, "unfused", 279620, 279620 + 7),
         ("unfused_vertical_only", 9, 35, 4, 35, "unfused", 34521, 2 * 34521 + 5),
         ("unfused_vertical_first_width_changes", 202, 2, 4, 3, "unfused", 13842, 13842 + 7)]


def _gather(base, n):
    """CUDA frame i = base[i % P]"""
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(base)).cuda()
    return dev[torch.arange(n, device="cuda") % P]


def _planar_padded(y, u, v, n):
    """planar, padding rows behind every frame of every plane"""
    import torch
    _, h, w = y.shape
    _, ch, cw = u.shape
    by = torch.full((n, h + 3, w), FILL, dtype=torch.uint8, device="cuda")
    bu, bv = (torch.full((n, ch + 2, cw), FILL, dtype=torch.uint8, device="cuda") for _ in range(2))
    vy, vu, vv = by[:, :h], bu[:, :ch], bv[:, :ch]
    y_fs, c_fs = vy.stride(0), vu.stride(0)
    assert 4 * c_fs != y_fs and c_fs != y_fs // 4 and c_fs != ch * cw and c_fs != y_fs and y_fs != h * w
    return (vy, vu, vv), (by, bu, bv)


def _nv12_cut(y, u, v, n):
    """interleaved chroma, every plane cut out of a larger allocation"""
    import torch
    _, h, w = y.shape
    _, ch, cw = u.shape
    by = torch.full((n + 2, h + 2, w + 5), FILL, dtype=torch.uint8, device="cuda")
    buv = torch.full((n + 2, ch + 2, cw + 3, 2), FILL, dtype=torch.uint8, device="cuda")
    vy = by[1:1 + n, 1:1 + h, 3:3 + w]
    vu, vv = buv[1:1 + n, 1:1 + ch, 1:1 + cw, 0], buv[1:1 + n, 1:1 + ch, 1:1 + cw, 1]
    assert vu.stride(2) == 2 and vv.data_ptr() == vu.data_ptr() + 1 and vu.stride(0) != vy.stride(0)
    return (vy, vu, vv), (by, buv)


LAYOUTS = {"planar_padded_frames": _planar_padded, "nv12_cut": _nv12_cut}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name,h,w,H,W,way,piece,n", CASES, ids=[c[0] for c in CASES])
def test_every_frame_past_the_first_piece(native, name, h, w, H, W, way, piece, n, layout):
    import torch
    assert path(h, w, H, W) == way
    assert piece == {"unfused": unfused_chunk(h, w), "fused": fused_chunk(h, W), "one pass": MAX_CHUNK_FRAMES}[way]
    assert n > piece and piece % P != 0 and np.gcd(piece, P) == 1
    if name == "unfused_same_size":
        assert n > MAX_CHUNK_FRAMES and piece > MAX_CHUNK_FRAMES      # iiv_resize_frames' own slices, inside one conversion chunk
    if name == "unfused_vertical_first_width_changes":
        assert resize_model.vertical_first(h, w) and W != w and H != h
    base = yuv_model.random_planes(P, h, w, seed=100 * h + w)
    exp = resize_model.resize(yuv_model.to_rgb(*base), (H, W))
    views, buffers = LAYOUTS[layout](*base, n)
    for view, plane in zip(views, base):
        view.copy_(_gather(plane, n))
    out = native.resize_frames_yuv420(*views, (H, W))
    assert tuple(out.shape) == (n, H, W, 3)
    _check_periodic(out, exp)
    del out, views, buffers
    torch.cuda.empty_cache()
