"""ctypes binding of libiivision.so (include/iivision.h).

PyTorch is plumbing here: it owns device memory (torch tensors whose data_ptr()
is handed to the C ABI) and the HIP stream.  There is no CPU fallback: if the
library or a GPU is missing, every compute entry point raises.
"""

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IIV_LIB") or os.path.join(os.path.dirname(_HERE), "libiivision.so")

HGR = 0
DHGR = 1

OK = 0
ERR_INVALID, ERR_HIP, ERR_NO_DEVICE, ERR_ASSERT, ERR_OVERFLOW = -1, -2, -3, -4, -5

STATE_MEM_MAIN, STATE_MEM_AUX, STATE_UP_MAIN, STATE_UP_AUX = 0, 1, 2, 3
STATE_RNG_PY, STATE_RNG_NP, STATE_OUT_OF_WORK, STATE_PACKED, STATE_COUNTERS = 4, 5, 6, 7, 8
OPT_DIFF_WEIGHTS, DW_TABLE, DW_RECURRENCE, DW_SPLIT = 1, 0, 1, 2
OPT_GREEDY_KERNEL, GREEDY_WAVE, GREEDY_WORKGROUP, GREEDY_AUTO, GREEDY_TEAM = 2, 0, 1, 2, 3
GREEDY_WAVE_SHARED, GREEDY_WAVE_PLAIN = 4, 5
OPT_PREFIX_SORT = 3
OPT_GREEDY_LDS_PAD = 5
OPT_CONTENT_CHOICE, CONTENT_TARGET, CONTENT_JOINT, CONTENT_JOINT_SPLIT = 6, 0, 1, 2
OPT_FOURTH_OFFSET = 7
OPT_STREAM_ORDER = 8


class Segment(C.Structure):
    _fields_ = [("frame", C.c_int32), ("is_aux", C.c_int32), ("restart", C.c_int32), ("n_ops", C.c_int32)]


class VideoState(C.Structure):
    """include/iivision.h: iiv_video_state"""
    _fields_ = [("mem_main", C.c_uint8 * 8192), ("mem_aux", C.c_uint8 * 8192),
                ("up_main", C.c_int32 * 8192), ("up_aux", C.c_int32 * 8192),
                ("rng_py", C.c_uint32 * 625), ("rng_np", C.c_uint32 * 625),
                ("out_of_work", C.c_int32 * 2), ("packed", C.c_uint64 * 4096)]

    def array(self, name, dtype, shape):
        return np.frombuffer(getattr(self, name), dtype=dtype).reshape(shape)


class VideoBrief(C.Structure):
    """include/iivision.h: iiv_video_brief"""
    _fields_ = [("priority_sum", C.c_int64 * 2), ("hole_bytes", C.c_int32 * 2), ("out_of_work", C.c_int32 * 2),
                ("rng_py", C.c_uint32 * 625), ("rng_np", C.c_uint32 * 625)]


class IIVError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libiivision error %d: %s" % (code, msg))
        self.code = code


class IIVAssertionError(AssertionError):
    """One of the reference's `assert`s fired on the device."""


_vp, _i32, _sz, _lg, _u16 = C.c_void_p, C.c_int, C.c_size_t, C.c_long, C.c_uint16

# The C ABI, declared once: name -> (restype, argtypes) of every function of include/iivision.h, in the header's order.
# tests/test_abi.py compares each entry with the header's prototype; lib() applies them.
_SIGNATURES = {
    "iiv_version": (C.c_char_p, []),
    "iiv_last_error": (C.c_char_p, []),
    "iiv_device_count": (_i32, []),
    # ---- mode constants
    "iiv_masked_bits": (_i32, [_i32]),
    "iiv_masked_dots": (_i32, [_i32]),
    "iiv_num_offsets": (_i32, [_i32]),
    "iiv_table_entries": (_sz, [_i32]),
    "iiv_store_table_entries": (_sz, [_i32]),
    # ---- P1: make_data_tables
    "iiv_cie2000_matrix": (_i32, [_vp, _vp, _vp, _vp]),
    "iiv_delta_e_cie2000": (_i32, [_i32, _vp, _vp, _vp, _vp]),
    "iiv_pixel_strings": (_i32, [_i32, _vp, _vp, _vp]),
    "iiv_build_table": (_i32, [_i32, _vp, _vp, _i32, _vp]),
    "iiv_build_store_table": (_i32, [_i32, _vp, _vp, _vp]),
    "iiv_symmetrise_table": (_i32, [_i32, _vp, _vp]),
    "iiv_store_table_from_table": (_i32, [_i32, _vp, _vp, _vp]),
    # ---- P2: screen.Bitmap operations
    "iiv_pack": (_i32, [_i32, _i32, _vp, _vp, _vp, _vp]),
    "iiv_diff_weights": (_i32, [_i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp]),
    "iiv_compute_delta_pages": (_i32, [_i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    # ---- P3: video.Video
    "iiv_build_split_store_table": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp]),
    "iiv_split_table_entries": (_sz, [_i32, _i32]),
    "iiv_build_narrow_store_table": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp]),
    "iiv_check_split_diff_table": (_i32, [_i32, _vp, _vp, _vp, _vp]),
    "iiv_check_diff_weight_pieces": (_i32, [_i32, _vp, _vp, _vp, _vp]),
    "iiv_encoder_create": (_i32, [_i32, _vp, _vp, _vp, _i32, C.POINTER(_vp)]),
    "iiv_encoder_destroy": (None, [_vp]),
    "iiv_encoder_set_option": (_i32, [_vp, _i32, _i32]),
    "iiv_encoder_info": (_i32, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "iiv_encoder_get_state": (_i32, [_vp, _i32, _i32, _vp, _sz]),
    "iiv_encoder_set_state": (_i32, [_vp, _i32, _i32, _vp, _sz]),
    "iiv_encoder_set_state_async": (_i32, [_vp, _i32, _i32, _vp, _sz, _vp]),
    "iiv_encoder_set_state_range": (_i32, [_vp, _i32, _i32, _i32, _vp, _sz]),
    "iiv_encoder_get_video_state": (_i32, [_vp, _i32, C.POINTER(VideoState)]),
    "iiv_encoder_set_video_state": (_i32, [_vp, _i32, C.POINTER(VideoState)]),
    "iiv_encoder_get_video_brief": (_i32, [_vp, _i32, C.POINTER(VideoBrief)]),
    "iiv_encoder_get_video_brief_async": (_i32, [_vp, _i32, C.POINTER(VideoBrief), _vp]),
    "iiv_encoder_snapshot": (_i32, [_vp, _vp]),
    "iiv_encoder_rollback": (_i32, [_vp, _vp]),
    "iiv_encoder_snapshot_slot": (_i32, [_vp, _i32, _vp]),
    "iiv_encoder_rollback_slot": (_i32, [_vp, _i32, _vp]),
    "iiv_encode": (_i32, [_vp, _vp, _vp, _i32, C.POINTER(Segment), _i32, _vp, _vp]),
    "iiv_encode_streams": (_i32, [_vp, _vp, _vp, _i32, C.POINTER(Segment), C.POINTER(C.c_int32), _vp, _sz, _vp]),
    "iiv_encoder_live_queue": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(C.c_int)]),
    "iiv_encode_live": (_i32, [_vp, _vp, _vp, _i32, C.POINTER(Segment), _i32, _vp, _i32, C.c_uint32, _vp]),
    "iiv_encoder_check": (_i32, [_vp, C.POINTER(C.c_int), _vp]),
    "iiv_encoder_profile": (_i32, [_vp, _i32]),
    "iiv_encoder_profile_read": (_i32, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "iiv_encoder_input_stats": (_i32, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "iiv_encoder_launch_forms": (_i32, [_vp, C.POINTER(C.c_int64)]),
    # ---- f2: byte emission
    "iiv_emit_stream": (_i32, [_i32, _i32, _lg, _vp, _vp, _vp, _u16, _u16, _lg, _vp, _sz, C.POINTER(_sz), _vp]),
    # ---- f3: frame ingest (the header declares f2's slice emission behind it)
    "iiv_frames_to_memory_maps": (_i32, [_i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "iiv_frames_to_memory_maps_diffused": (_i32, [_i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "iiv_emit_chunk": (_i32, [_i32, _i32, _lg, _lg, _vp, _sz, _vp, _sz, _i32, _vp, _u16, _vp, _sz,
                              C.POINTER(_sz), C.POINTER(_sz), _vp, _vp]),
    # ---- f4: the audio track
    "iiv_audio_tick_count": (_lg, [_lg, _i32, _i32, _lg]),
    "iiv_audio_ticks": (_i32, [_i32, _vp, _sz, _vp, _vp, _vp, _i32, _lg, _vp, _vp, _sz, _vp, _vp]),
    "iiv_audio_resample": (_i32, [_i32, _vp, _sz, _vp, _vp, _vp, _i32, _vp, _sz, _vp, _vp]),
    "iiv_audio_normalization": (_i32, [_i32, _vp, _sz, _vp, _vp, _vp, _i32, _vp, _vp]),
    # ---- f5: the resize
    "iiv_resize_coeffs": (_i32, [_i32, _i32, C.POINTER(C.c_int), _vp, _vp]),
    "iiv_resize_frames": (_i32, [_i32, _i32, _i32, _vp, _sz, _sz, _i32, _i32, _vp, _vp]),
    # ---- f6: mono playback mode
    "iiv_frames_to_memory_maps_mono": (_i32, [_i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    # ---- f7: preview
    "iiv_render_rgb": (_i32, [_i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "iiv_encoder_render": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp]),
    # ---- f8: screen error
    "iiv_render_error": (_i32, [_i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "iiv_encoder_render_error": (_i32, [_vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp]),
    # ---- f9: reading an opcode stream
    "iiv_a2m_reader_create": (_i32, [_vp, _u16, _u16, C.POINTER(_vp)]),
    "iiv_a2m_reader_destroy": (None, [_vp]),
    "iiv_a2m_max_ops": (_lg, [_sz]),
    "iiv_a2m_scan": (_i32, [_vp, _i32, _vp, _sz, _vp, _vp, _vp]),
    "iiv_a2m_decode": (_i32, [_vp, _i32, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _vp]),
    "iiv_a2m_replay": (_i32, [_vp, _i32, _vp, _sz, _vp, _lg, _lg, _i32, _vp, _vp, _vp, _vp, _vp]),
    # ---- f10: direct ingest
    "iiv_frames_to_memory_maps_direct": (_i32, [_i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    # ---- f11: YUV 4:2:0 sources
    "iiv_resize_frames_yuv420": (_i32, [_i32, _i32, _i32, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _i32, _vp, _i32, _i32, _vp, _vp]),
    # ---- f12: boxed resize, letterbox and crop
    "iiv_resize_coeffs_box": (_i32, [_i32, _vp, _i32, C.POINTER(C.c_int), _vp, _vp]),
    "iiv_resize_frames_fit": (_i32, [_i32, _i32, _i32, _vp, _sz, _sz, _vp, _i32, _i32, _vp, C.c_uint32, _vp, _vp]),
    "iiv_resize_frames_yuv420_fit": (_i32, [_i32, _i32, _i32, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _i32, _vp, _vp, _i32, _i32, _vp,
                                            C.c_uint32, _vp, _vp]),
    # ---- f13: speaker preview
    "iiv_speaker_periods": (_lg, [_lg]),
    "iiv_speaker_sample_count": (_lg, [_lg, _i32]),
    "iiv_speaker_pcm": (_i32, [_i32, _vp, _sz, _vp, _sz, _i32, _i32, _i32, _vp, _sz, _vp, _vp]),
    # ---- f14: temporal hold
    "iiv_temporal_hold": (_i32, [_i32, _i32, _lg, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _sz, _i32, _i32, _i32, _vp, _vp]),
    # ---- f15: picture levels
    "iiv_levels_histogram": (_i32, [_i32, _i32, _lg, _vp, _sz, _sz, _vp, _vp]),
    "iiv_levels_auto": (_i32, [_vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "iiv_levels_apply": (_i32, [_i32, _i32, _lg, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _sz, _vp]),
    # ---- f16: spatial filter
    "iiv_filter_frames": (_i32, [_i32, _i32, _i32, _i32, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
}
SYMBOLS = list(_SIGNATURES)

_lib = None


def lib():
    """Load libiivision.so and declare every function of _SIGNATURES on it; fails loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not found: build it with `make -C ii-vision_amd/csrc` "
            "(or python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback." % LIB_PATH)
    # torch bundles its own HIP runtime (SONAME libamdhip64.so.7).  Import it first so
    # that our NEEDED entry resolves to that already-loaded copy: two HIP/HSA runtimes
    # in one process cannot both own the device.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _SIGNATURES.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            if "IIV_LIB" in os.environ:   # an A/B run against an older build (tools/ab_libs.sh) does without it
                continue
            raise AttributeError("%s does not export %s, which include/iivision.h declares" % (LIB_PATH, name)) from None
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def build_id():
    """The library's build id (include/iivision.h: iiv_version): a hash of the sources and flags it was built from."""
    v = lib().iiv_version().decode("ascii", "replace")
    return v.split(" build ", 1)[1] if " build " in v else "unknown"


def check(rc):
    if rc == OK:
        return
    msg = lib().iiv_last_error().decode("utf-8", "replace")
    if rc == ERR_ASSERT:
        raise IIVAssertionError(msg)
    raise IIVError(rc, msg)


_torch_mod = None


def _torch():
    global _torch_mod
    if _torch_mod is not None:   # (availability was established once; the check costs microseconds per call)
        return _torch_mod
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("libiivision needs an AMD GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback")
    _torch_mod = torch
    return torch


def stream_ptr():
    """torch's current stream on the current device, as a raw hipStream_t"""
    torch = _torch()
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:   # the same value as current_stream().cuda_stream without building a Stream object
        return C.c_void_p(raw(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def hptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- P1 -------------------------------------------------------------------------

def cie2000_matrix(rgb):
    """rgb: (16,3) uint8 indexed by HGRColours value -> (float64 (16,16), int32 (16,16))."""
    _torch()
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(48)
    f = np.zeros((16, 16), dtype=np.float64)
    i = np.zeros((16, 16), dtype=np.int32)
    check(lib().iiv_cie2000_matrix(hptr(rgb), hptr(f), hptr(i), stream_ptr()))
    return f, i


def delta_e_cie2000(lab1, lab2):
    """Delta-E 2000 of (n, 3) Lab pairs on the device (the table builder's own function)."""
    _torch()
    a = np.ascontiguousarray(lab1, dtype=np.float64).reshape(-1, 3)
    b = np.ascontiguousarray(lab2, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(a), dtype=np.float64)
    check(lib().iiv_delta_e_cie2000(len(a), hptr(a), hptr(b), hptr(out), stream_ptr()))
    return out


def pixel_strings(mode):
    torch = _torch()
    L = lib()
    n = L.iiv_num_offsets(mode) << L.iiv_masked_bits(mode)
    nd = L.iiv_masked_dots(mode)
    dots = torch.empty(n, dtype=torch.int32, device="cuda")
    pix = torch.empty((n, nd), dtype=torch.uint8, device="cuda")
    check(L.iiv_pixel_strings(mode, dptr(dots), dptr(pix), stream_ptr()))
    shape = (L.iiv_num_offsets(mode), 1 << L.iiv_masked_bits(mode))
    return dots.view(shape), pix.view(shape + (nd,))


def _diff_matrix(dm):
    """The 16x16 int diff matrix as the C ABI takes it: const int32_t dm[256]."""
    return np.ascontiguousarray(dm, dtype=np.int32).reshape(256)


def build_table(mode, dm, symmetric=True):
    """Device tensor (num_offsets, 2**(2*bits)) int16-typed storage of the u16 table."""
    torch = _torch()
    L = lib()
    dm = _diff_matrix(dm)
    bits = L.iiv_masked_bits(mode)
    out = torch.empty((L.iiv_num_offsets(mode), 1 << (2 * bits)), dtype=torch.int16, device="cuda")
    check(L.iiv_build_table(mode, hptr(dm), dptr(out), 1 if symmetric else 0, stream_ptr()))
    return out


def build_store_table(mode, dm):
    torch = _torch()
    L = lib()
    dm = _diff_matrix(dm)
    out = torch.empty(L.iiv_store_table_entries(mode), dtype=torch.int16, device="cuda")
    check(L.iiv_build_store_table(mode, hptr(dm), dptr(out), stream_ptr()))
    return out


def check_split_diff_table(mode, dm, table):
    """Number of entries of the full symmetric table that differ from the combination of the
    two halves of the split diff-weight table built from dm (0 = exact everywhere)."""
    _torch()
    dm = _diff_matrix(dm)
    n = C.c_ulonglong(0)
    check(lib().iiv_check_split_diff_table(mode, hptr(dm), dptr(table), C.byref(n), stream_ptr()))
    return int(n.value)


def check_diff_weight_pieces(mode, dm, table):
    """Entries of the full symmetric table that differ from the sum of pixel-pair terms the prologue
    evaluates instead of the recurrence (include/iivision.h: iiv_check_diff_weight_pieces); both modes."""
    dm = _diff_matrix(dm)
    n = C.c_ulonglong(0)
    check(lib().iiv_check_diff_weight_pieces(mode, hptr(dm), dptr(table), C.byref(n), stream_ptr()))
    return int(n.value)


def build_narrow_store_table(mode, dm, store):
    """(expanded, n_mismatch): every store value as the greedy kernels obtain it from the narrow
    form of the split table (S = L1 + RF, two u16 tables), and the number of entries that differ
    from `store` (0 when both come from the same dm)."""
    torch = _torch()
    dm = _diff_matrix(dm)
    exp = torch.empty_like(store)
    n = C.c_ulonglong(0)
    check(lib().iiv_build_narrow_store_table(mode, hptr(dm), dptr(store), dptr(exp), C.byref(n), stream_ptr()))
    return exp, int(n.value)


def build_split_store_table(mode, dm, expanded=True):
    """(left, right, expanded) device tensors: the two halves of the split store table and
    (optionally) the dense store table rebuilt from them with the encoder's index arithmetic."""
    torch = _torch()
    L = lib()
    dm = _diff_matrix(dm)
    left = torch.empty(L.iiv_split_table_entries(mode, 0), dtype=torch.int32, device="cuda")
    right = torch.empty(L.iiv_split_table_entries(mode, 1), dtype=torch.int32, device="cuda")
    exp = torch.empty(L.iiv_store_table_entries(mode), dtype=torch.int16, device="cuda") if expanded else None
    check(L.iiv_build_split_store_table(mode, hptr(dm), dptr(left), dptr(right), dptr(exp), stream_ptr()))
    return left, right, exp


def load_table(mode, lower_or_file_array):
    """A table as a reference .npz holds it (lower triangle) -> (symmetric table, store table) in HBM:
    Bitmap.edit_distances' load + mirror (screen.py:343-367) on the device."""
    torch = _torch()
    L = lib()
    bits = L.iiv_masked_bits(mode)
    a = np.ascontiguousarray(lower_or_file_array, dtype=np.uint16)
    if a.shape != (L.iiv_num_offsets(mode), 1 << (2 * bits)):
        raise ValueError("edit_distance array has shape %s, expected %s" % (a.shape, (L.iiv_num_offsets(mode), 1 << (2 * bits))))
    table = torch.from_numpy(a.view(np.int16)).cuda()
    check(L.iiv_symmetrise_table(mode, dptr(table), stream_ptr()))
    store = torch.empty(L.iiv_store_table_entries(mode), dtype=torch.int16, device="cuda")
    check(L.iiv_store_table_from_table(mode, dptr(table), dptr(store), stream_ptr()))
    return table, store


def table_to_numpy(t):
    """u16 view of a table tensor on the host."""
    return t.cpu().numpy().view(np.uint16)


# ---- P2 -------------------------------------------------------------------------

def pack(mode, main_mem, aux_mem=None):
    """main/aux: uint8 arrays (..., 32, 256) on host -> uint64 (..., 32, 128) on host."""
    torch = _torch()
    main_mem = np.ascontiguousarray(main_mem, dtype=np.uint8)
    lead = main_mem.shape[:-2]
    n = int(np.prod(lead)) if lead else 1
    dm_ = torch.from_numpy(main_mem.reshape(n, 32, 256)).cuda()
    da = None
    if mode == DHGR:
        da = torch.from_numpy(np.ascontiguousarray(aux_mem, dtype=np.uint8).reshape(n, 32, 256)).cuda()
    out = torch.empty((n, 32, 128), dtype=torch.int64, device="cuda")
    check(lib().iiv_pack(mode, n, dptr(dm_), dptr(da), dptr(out), stream_ptr()))
    return out.cpu().numpy().view(np.uint64).reshape(lead + (32, 128))


def diff_weights(mode, table, src_packed, tgt_packed, is_aux):
    """src/tgt: uint64 arrays (..., 32, 128) on host, screen k against screen k -> int32 (..., 32, 256) on host."""
    torch = _torch()
    src_packed = np.ascontiguousarray(src_packed, dtype=np.uint64)
    tgt_packed = np.ascontiguousarray(tgt_packed, dtype=np.uint64)
    if src_packed.shape != tgt_packed.shape or src_packed.shape[-2:] != (32, 128):
        raise ValueError("packed source %s and target %s must both be (..., 32, 128)" % (src_packed.shape, tgt_packed.shape))
    lead = src_packed.shape[:-2]
    n = int(np.prod(lead)) if lead else 1
    src = torch.from_numpy(src_packed.view(np.int64).reshape(n, 32, 128)).cuda()
    tgt = torch.from_numpy(tgt_packed.view(np.int64).reshape(n, 32, 128)).cuda()
    out = torch.empty((n, 32, 256), dtype=torch.int32, device="cuda")
    check(lib().iiv_diff_weights(mode, dptr(table), n, dptr(src), dptr(tgt), int(bool(is_aux)), dptr(out),
                                 stream_ptr()))
    return out.cpu().numpy().reshape(lead + (32, 256))


def compute_delta_pages(mode, table, tgt_packed, pages, contents, dw_rows, is_aux):
    torch = _torch()
    tgt = torch.from_numpy(np.ascontiguousarray(tgt_packed, dtype=np.uint64).view(np.int64)).cuda()
    pages = np.ascontiguousarray(pages, dtype=np.int32).reshape(-1)
    n = len(pages)
    dp = torch.from_numpy(pages).cuda()
    dc = torch.from_numpy(np.ascontiguousarray(contents, dtype=np.int32).reshape(-1)).cuda()
    dr = torch.from_numpy(np.ascontiguousarray(dw_rows, dtype=np.int32).reshape(n, 256)).cuda()
    out = torch.empty((n, 256), dtype=torch.int32, device="cuda")
    check(lib().iiv_compute_delta_pages(mode, dptr(table), n, dptr(tgt), dptr(dp), dptr(dc), dptr(dr),
                                        int(bool(is_aux)), dptr(out), stream_ptr()))
    return out.cpu().numpy()


# ---- P3 -------------------------------------------------------------------------

def encoder_info(handle):
    """(mode, n_streams) of the encoder behind an iiv_encoder* (iiv_encoder_info): what its callers' buffers must be sized for."""
    mode, n = C.c_int(-1), C.c_int(0)
    check(lib().iiv_encoder_info(handle if isinstance(handle, C.c_void_p) else C.c_void_p(int(handle)), C.byref(mode), C.byref(n)))
    return mode.value, n.value


def _cuda_u8(t, name):
    """ValueError unless t is a contiguous CUDA uint8 tensor."""
    torch = _torch_mod or _torch()
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous CUDA uint8 tensor" % name)


def _frames_bank(t, name, n_streams):
    """ValueError unless t is one bank of target frames, (n_streams, n_frames, 32, 256), as validate_frames wants it."""
    _cuda_u8(t, name)
    if t.dim() != 4 or tuple(t.shape[2:]) != (32, 256):
        raise ValueError("%s has shape %s, not (n_streams, n_frames, 32, 256)" % (name, tuple(t.shape)))
    if int(t.shape[0]) != n_streams:
        raise ValueError("%s holds %d streams, the encoder was created for %d" % (name, int(t.shape[0]), n_streams))


def validate_frames(handle, frames_main, frames_aux):
    """iiv_encode / iiv_encode_streams read n_streams x n_frames x 8192 bytes of every bank whatever the caller's tensors
    hold: refuse anything else here instead of letting a kernel read out of bounds.  Returns (n_streams, n_frames)."""
    mode, n_streams = encoder_info(handle)
    _frames_bank(frames_main, "frames_main", n_streams)
    n_frames = int(frames_main.shape[1])
    if n_frames <= 0:
        raise ValueError("frames_main holds no frame")
    if mode == DHGR:
        if frames_aux is None:
            raise ValueError("DHGR needs frames_aux")
        _frames_bank(frames_aux, "frames_aux", n_streams)
        if int(frames_aux.shape[1]) != n_frames:
            raise ValueError("frames_aux holds %d frames per stream, frames_main %d" % (int(frames_aux.shape[1]), n_frames))
    elif frames_aux is not None:
        _frames_bank(frames_aux, "frames_aux", n_streams)   # (HGR ignores it; a tensor of the wrong kind is still a caller's mistake)
    return n_streams, n_frames


def validate_ops_out(ops_out, need_bytes):
    _cuda_u8(ops_out, "ops_out")
    if ops_out.numel() < need_bytes:
        raise ValueError("ops_out holds %d bytes, this call writes %d (n_streams * total opcodes * 6)" % (ops_out.numel(), need_bytes))


def segment_array(segments):
    """[(frame, is_aux, restart, n_ops), ...] -> the iiv_segment array of the C ABI (never of length 0: ctypes needs one entry)."""
    return (Segment * max(len(segments), 1))(*[Segment(int(f), int(a), int(r), int(k)) for (f, a, r, k) in segments])


def _state_array(what, value, n=None):
    """`value` as the C ABI takes state item `what`: its dtype and shape (Encoder._ITEMS), n of them back to back if n is given."""
    shape, dt = Encoder._ITEMS[what]
    return np.ascontiguousarray(value, dtype=dt).reshape(shape if n is None else (n,) + shape)


class Encoder:
    """n_streams independent video.Video states resident on the GPU."""

    def __init__(self, mode, table, store_table, n_streams=1, dm=None):
        """dm: the 16x16 int diff matrix the tables came from; if given, diff weights
        are recomputed by recurrence instead of gathered from `table` (same values)."""
        _torch()
        self.mode = mode
        self.n_streams = int(n_streams)
        self._table = table            # keep the device tensors alive
        self._store = store_table
        h = C.c_void_p()
        dmp = C.c_void_p(0)
        if dm is not None:
            self._dm = _diff_matrix(dm)
            dmp = hptr(self._dm)
        check(lib().iiv_encoder_create(mode, dptr(table), dptr(store_table), dmp, self.n_streams, C.byref(h)))
        self._h = h

    @property
    def handle(self):
        """The iiv_encoder* as an int: what torch.ops.iivision.encode / encode_streams take (torch_ops.py)."""
        return int(self._h.value)

    def set_greedy_kernel(self, wave_per_stream):
        """True: one wave per stream; False: one 256-thread workgroup; "team": eight waves per stream;
        "shared" / "plain": one wave per stream with / without the bank's L1 table half shared in LDS by
        the eight streams of a workgroup (True picks by batch size); None: automatic."""
        names = {None: GREEDY_AUTO, "auto": GREEDY_AUTO, "team": GREEDY_TEAM, "shared": GREEDY_WAVE_SHARED, "plain": GREEDY_WAVE_PLAIN,
                 "wave": GREEDY_WAVE, "workgroup": GREEDY_WORKGROUP}
        if wave_per_stream is None or isinstance(wave_per_stream, str):
            if wave_per_stream not in names:
                raise ValueError("set_greedy_kernel: unknown kernel %r (one of %s, True, False, None)"
                                 % (wave_per_stream, ", ".join(repr(k) for k in names if k)))
            v = names[wave_per_stream]
        else:
            v = GREEDY_WAVE if wave_per_stream else GREEDY_WORKGROUP
        check(lib().iiv_encoder_set_option(self._h, OPT_GREEDY_KERNEL, v))

    def set_stream_order(self, enable):
        """True (default): big batches launch the one-wave kernel longest stream first (IIV_OPT_STREAM_ORDER); same bytes."""
        check(lib().iiv_encoder_set_option(self._h, OPT_STREAM_ORDER, 1 if enable else 0))

    def set_prefix_sort(self, enable):
        check(lib().iiv_encoder_set_option(self._h, OPT_PREFIX_SORT, 1 if enable else 0))

    def set_greedy_lds_pad(self, n_bytes):
        check(lib().iiv_encoder_set_option(self._h, OPT_GREEDY_LDS_PAD, int(n_bytes)))

    def set_content_choice(self, joint):
        """False (default): the reference's greedy step.  True: the content byte of every step is
        chosen jointly with its extra offsets (include/iivision.h: IIV_CONTENT_JOINT) -- the
        reference README's "global optimization" idea, NOT the reference's output.  "split": the same choice
        computed by the slower second implementation (IIV_CONTENT_JOINT_SPLIT)."""
        value = CONTENT_JOINT_SPLIT if joint == "split" else CONTENT_JOINT if joint else CONTENT_TARGET
        check(lib().iiv_encoder_set_option(self._h, OPT_CONTENT_CHOICE, value))

    def set_fourth_offset(self, enable):
        """f4: up to three extra offsets per opcode instead of two and a copy of the first (the reference's exit test
        `len(offsets) == 3`, video.py:180-181, read as 4; include/iivision.h IIV_OPT_FOURTH_OFFSET).  NOT the
        reference's opcode stream."""
        check(lib().iiv_encoder_set_option(self._h, OPT_FOURTH_OFFSET, 1 if enable else 0))

    def set_diff_weights_mode(self, mode):
        """True / "recurrence" (default with dm): the edit-distance recurrence in the kernel;
        "split": two gathers from the split diff-weight table; False / "table": one gather from
        the full table."""
        v = {"split": DW_SPLIT, "recurrence": DW_RECURRENCE, "table": DW_TABLE, True: DW_RECURRENCE,
             False: DW_TABLE}[mode]
        check(lib().iiv_encoder_set_option(self._h, OPT_DIFF_WEIGHTS, v))

    def close(self):
        if getattr(self, "_h", None):
            lib().iiv_encoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _ITEMS = {
        STATE_MEM_MAIN: ((32, 256), np.uint8), STATE_MEM_AUX: ((32, 256), np.uint8),
        STATE_UP_MAIN: ((32, 256), np.int32), STATE_UP_AUX: ((32, 256), np.int32),
        STATE_RNG_PY: ((625,), np.uint32), STATE_RNG_NP: ((625,), np.uint32),
        STATE_OUT_OF_WORK: ((2,), np.int32), STATE_PACKED: ((32, 128), np.uint64),
        STATE_COUNTERS: ((4,), np.uint64),
        100: ((32,), np.uint64),  # phase stamps of diagnostic (-DIIV_STAMPS) builds
    }

    def get_state(self, what, stream=0, out=None):
        shape, dt = self._ITEMS[what]
        if out is None:
            out = np.empty(shape, dtype=dt)
        assert out.flags.c_contiguous and out.dtype == dt and out.shape == shape
        check(lib().iiv_encoder_get_state(self._h, int(stream), what, hptr(out), out.nbytes))
        return out

    def set_state(self, what, value, stream=0):
        a = _state_array(what, value)
        check(lib().iiv_encoder_set_state(self._h, int(stream), what, hptr(a), a.nbytes))

    def set_state_async(self, what, value, stream=0):
        """STATE_OUT_OF_WORK / STATE_RNG_PY / STATE_RNG_NP of one stream, enqueued behind the launches already on the current
        HIP stream: no device-wide synchronisation (iiv_encoder_set_state_async)."""
        shape, dt = self._ITEMS[what]   # (_state_array, written out: the drop-in Video calls this once per generator)
        a = np.ascontiguousarray(value, dtype=dt).reshape(shape)
        check(lib().iiv_encoder_set_state_async(self._h, int(stream), what, hptr(a), a.nbytes, stream_ptr()))

    def get_video_state(self, stream=0, out=None):
        out = out if out is not None else VideoState()
        check(lib().iiv_encoder_get_video_state(self._h, int(stream), C.byref(out)))
        return out

    def get_video_brief(self, stream=0, out=None):
        out = out if out is not None else VideoBrief()
        check(lib().iiv_encoder_get_video_brief(self._h, int(stream), C.byref(out)))
        return out

    def get_video_brief_async(self, out, stream=0):
        """The brief of the state as it will be behind the launches already enqueued, copied into `out` (a VideoBrief in
        pinned memory) by the time the stream is synchronised (check())."""
        check(lib().iiv_encoder_get_video_brief_async(self._h, int(stream), C.byref(out), stream_ptr()))

    def set_video_state(self, state, stream=0):
        check(lib().iiv_encoder_set_video_state(self._h, int(stream), C.byref(state)))

    def set_state_all(self, what, values, first=0):
        """values: (n, ...) array, item `what` of streams first .. first + n - 1 in one upload."""
        n = np.shape(values)[0]
        a = _state_array(what, values, n)
        check(lib().iiv_encoder_set_state_range(self._h, int(first), n, what, hptr(a), a[0].nbytes))

    def encode_streams(self, frames_main, frames_aux, schedules, ops_out=None):
        """Per-stream schedules: schedules[s] = list of (frame, is_aux, restart, n_ops) of stream s.
        Returns (ops tensor (n_streams, max total, 6), per-stream totals).  Asynchronous."""
        torch = _torch()
        _, n_frames = validate_frames(self._h, frames_main, frames_aux)
        if len(schedules) != self.n_streams:
            raise ValueError("%d schedules for %d streams" % (len(schedules), self.n_streams))
        flat = [g for sch in schedules for g in sch]
        segs = segment_array(flat)
        begin = np.zeros(self.n_streams + 1, dtype=np.int32)
        begin[1:] = np.cumsum([len(sch) for sch in schedules])
        totals = [sum(int(g[3]) for g in sch) for sch in schedules]
        width = max(max(totals), 1)
        if ops_out is None:
            ops_out = torch.zeros((self.n_streams, width, 6), dtype=torch.uint8, device="cuda")
        if ops_out.dim() != 3 or int(ops_out.shape[0]) != self.n_streams or int(ops_out.shape[2]) != 6 or int(ops_out.shape[1]) < width:
            raise ValueError("ops_out has shape %s, this call needs (%d, >= %d, 6)" % (tuple(ops_out.shape), self.n_streams, width))
        validate_ops_out(ops_out, self.n_streams * width * 6)
        stride = ops_out.shape[1] * 6
        check(lib().iiv_encode_streams(self._h, dptr(frames_main), dptr(frames_aux), int(n_frames), segs,
                                       begin.ctypes.data_as(C.POINTER(C.c_int32)), dptr(ops_out), stride, stream_ptr()))
        return ops_out, totals

    def encode(self, frames_main, frames_aux, segments, ops_out=None):
        """frames_*: CUDA uint8 tensors (n_streams, n_frames, 32, 256); segments: list of
        (frame, is_aux, restart, n_ops).  Returns the CUDA uint8 tensor
        (n_streams, total_ops, 6).  Asynchronous."""
        torch = _torch()
        _, n_frames = validate_frames(self._h, frames_main, frames_aux)
        segs = segment_array(segments)
        total = sum(int(s[3]) for s in segments)
        need = self.n_streams * total * 6
        if ops_out is None:
            ops_out = torch.empty((self.n_streams, total, 6), dtype=torch.uint8, device="cuda")
        else:
            # iiv_encode packs stream s at byte s * total * 6 whatever the shape of the caller's buffer: a
            # pre-allocated buffer may be larger than this call needs (calls of a Movie-paced driver differ
            # in their opcode count), never smaller -- that would be a device write out of bounds
            validate_ops_out(ops_out, need)
        check(lib().iiv_encode(self._h, dptr(frames_main), dptr(frames_aux), int(n_frames), segs, len(segments),
                               dptr(ops_out), stream_ptr()))
        # the rows as they were written: (n_streams, total, 6) over the front of the buffer
        return ops_out.view(-1)[:need].view(self.n_streams, total, 6)

    def live_queue(self, slot=0):
        """Queue `slot` of the live hand-over (include/iivision.h: iiv_encoder_live_queue) as a numpy uint64 view of the
        coherent host memory the team kernel writes its opcodes into: slot j = six opcode bytes | tag << 48."""
        addr, cap = C.c_void_p(0), C.c_int(0)
        check(lib().iiv_encoder_live_queue(self._h, int(slot), C.byref(addr), C.byref(cap)))
        return np.frombuffer((C.c_uint64 * cap.value).from_address(addr.value), dtype=np.uint64)

    def encode_live(self, frames_main, frames_aux, segment, ops_out, slot, tag):
        """iiv_encode_live of ONE segment (frame, is_aux, restart, n_ops): iiv_encode, the opcodes also appearing one by one
        in live_queue(slot) under `tag`.  Raises IIVError(ERR_INVALID) -- nothing launched -- if this encoder's options
        keep it off the team kernel."""
        _, n_frames = validate_frames(self._h, frames_main, frames_aux)
        f, a, r, k = segment
        seg = Segment(int(f), int(a), int(r), int(k))
        validate_ops_out(ops_out, self.n_streams * int(k) * 6)
        check(lib().iiv_encode_live(self._h, dptr(frames_main), dptr(frames_aux), int(n_frames), C.byref(seg), 1, dptr(ops_out),
                                    int(slot), int(tag), stream_ptr()))

    def snapshot(self, slot=0):
        check(lib().iiv_encoder_snapshot_slot(self._h, int(slot), stream_ptr()))

    def rollback(self, slot=0):
        check(lib().iiv_encoder_rollback_slot(self._h, int(slot), stream_ptr()))

    def check(self):
        bad = C.c_int(-1)
        check(lib().iiv_encoder_check(self._h, C.byref(bad), stream_ptr()))

    def profile(self, enable=True):
        check(lib().iiv_encoder_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        ms = (C.c_double * 2)()
        n = (C.c_int64 * 2)()
        check(lib().iiv_encoder_profile_read(self._h, ms, n))
        return {"prologue_ms": ms[0], "greedy_ms": ms[1], "prologue_launches": n[0], "greedy_launches": n[1]}

    def launch_forms(self):
        """Greedy launches since profile(True) by kernel: {"plain", "shared", "team", "workgroup"} (iiv_encoder_launch_forms)."""
        if not hasattr(lib(), "iiv_encoder_launch_forms"):   # (an older build under IIV_LIB, tools/ab_libs.sh)
            return None
        c = (C.c_int64 * 4)()
        check(lib().iiv_encoder_launch_forms(self._h, c))
        return {"plain": int(c[0]), "shared": int(c[1]), "team": int(c[2]), "workgroup": int(c[3])}

    def input_stats(self):
        """(share of the steps the nonces decided, as the kernels reported it for an earlier call; the form of the one-wave
        kernel the next full-batch launch runs: "shared" / "plain") -- include/iivision.h: iiv_encoder_input_stats"""
        st, form = (C.c_double * 2)(), C.c_int(0)
        check(lib().iiv_encoder_input_stats(self._h, st, C.byref(form)))
        self.real_opcodes_per_launch = st[1]
        return st[0], "shared" if form.value == GREEDY_WAVE_SHARED else "plain"


# ---- f2: byte emission -------------------------------------------------------------

def emit_stream_size(mode, n_ops, tick_addr, ack_addr, terminate_addr, max_bytes_out=None):
    ta = np.ascontiguousarray(tick_addr, dtype=np.uint16).reshape(1024)
    n = C.c_size_t(0)
    check(lib().iiv_emit_stream(mode, 1, int(n_ops), None, None, hptr(ta), int(ack_addr), int(terminate_addr),
                                int(max_bytes_out or 0), None, 0, C.byref(n), None))
    return int(n.value)


def emit_stream(mode, ops, ticks, tick_addr, ack_addr, terminate_addr, max_bytes_out=None):
    """ops: CUDA uint8 (S, n, 6); ticks: CUDA uint8 (S, n) -> CUDA uint8 (S, length)."""
    torch = _torch()
    S, n = int(ops.shape[0]), int(ops.shape[1])
    ta = np.ascontiguousarray(tick_addr, dtype=np.uint16).reshape(1024)
    length = emit_stream_size(mode, n, ta, ack_addr, terminate_addr, max_bytes_out)
    out = torch.empty((S, length), dtype=torch.uint8, device="cuda")
    got = C.c_size_t(0)
    ops_c, ticks_c = ops.contiguous(), ticks.contiguous()   # (kept in locals: the call reads their storage)
    check(lib().iiv_emit_stream(mode, S, n, dptr(ops_c), dptr(ticks_c), hptr(ta), int(ack_addr),
                                int(terminate_addr), int(max_bytes_out or 0), dptr(out), length, C.byref(got),
                                stream_ptr()))
    return out


def emit_chunk_range(mode, first_op, n_ops):
    """(first byte, byte count) of opcodes [first_op, first_op + n_ops) in a stream."""
    b0, nb = C.c_size_t(0), C.c_size_t(0)
    check(lib().iiv_emit_chunk(mode, 1, int(first_op), int(n_ops), None, 0, None, 0, 34, None, 0, None, 0,
                               C.byref(b0), C.byref(nb), None, None))
    return int(b0.value), int(nb.value)


def emit_chunk(mode, ops, first_op, d_tick_addr, ack_addr, out, ticks=None, const_tick=34, d_err=None):
    """Asynchronous slice emission.  ops: CUDA uint8 (S, n, 6) view (row stride arbitrary) holding opcodes
    first_op .. first_op + n - 1 of every stream; out: CUDA uint8 (S, >= byte count) -> (first byte, byte count)."""
    _torch()
    S, n = int(ops.shape[0]), int(ops.shape[1])
    assert ops.stride(2) == 1 and ops.stride(1) == 6 and out.stride(1) == 1
    b0, nb = C.c_size_t(0), C.c_size_t(0)
    check(lib().iiv_emit_chunk(mode, S, int(first_op), n, dptr(ops), int(ops.stride(0)), dptr(ticks),
                               int(ticks.stride(0)) if ticks is not None else 0, int(const_tick), dptr(d_tick_addr),
                               int(ack_addr), dptr(out), int(out.stride(0)), C.byref(b0), C.byref(nb), dptr(d_err),
                               stream_ptr()))
    return int(b0.value), int(nb.value)


# ---- f3: frame ingest ---------------------------------------------------------------

DITHER_DIFFUSION = 256   # IIV_DITHER_DIFFUSION: Floyd-Steinberg error diffusion instead of the ordered dither


def _memory_maps_out(mode, n, out):
    """The (main, aux) memory maps an ingest call writes: new (n, 32, 256) tensors, or the caller's out=(main, aux) once they
    are known to hold n * 8192 bytes each; aux is None for HGR."""
    torch = _torch()
    if out is None:
        main = torch.empty((n, 32, 256), dtype=torch.uint8, device="cuda")
        aux = torch.empty((n, 32, 256), dtype=torch.uint8, device="cuda") if mode == DHGR else None
        return main, aux
    main, aux = out
    for t in ((main, aux) if mode == DHGR else (main,)):
        _cuda_u8(t, "each out tensor")
        if t.numel() != n * 8192:
            raise ValueError("each out tensor must hold n * 8192 bytes")
    return main, aux if mode == DHGR else None


def frames_to_memory_maps(mode, palette_rgb, rgb, dither=0, out=None):
    """rgb: CUDA uint8 (n, 192, 280, 3) -> (main, aux) CUDA uint8 (n, 32, 256); aux is None for HGR.
    dither: 0..255 = amplitude of the 4x4 ordered dither, DITHER_DIFFUSION = error diffusion.
    out=(main, aux): write into these contiguous CUDA uint8 tensors of n * 8192 bytes each (any shape; aux ignored
    for HGR) instead of allocating -- e.g. a (streams, frames, 32, 256) slice of a batch's target frames.
    Asynchronous on torch's current stream (since round 5; it used to synchronise): `rgb` and the `out` tensors must stay
    alive and untouched until that stream has reached this call.  Tensors allocated and used on the same current stream are
    safe as they are (the caching allocator re-uses a freed block on that stream only behind its pending work); tensors
    that belong to ANOTHER stream -- a conversion on a side stream writing into the encoder's target buffers, as bench.py's
    e2e leg does -- need tensor.record_stream(torch.cuda.current_stream()) or an event between the streams."""
    _cuda_u8(rgb, "rgb")
    if tuple(rgb.shape[1:]) != (192, 280, 3):
        raise ValueError("rgb has shape %s, not (n, 192, 280, 3)" % (tuple(rgb.shape),))
    n = int(rgb.shape[0])
    pal = np.ascontiguousarray(palette_rgb, dtype=np.uint8).reshape(48)
    main, aux = _memory_maps_out(mode, n, out)
    check(lib().iiv_frames_to_memory_maps(mode, hptr(pal), n, dptr(rgb), int(dither), dptr(main), dptr(aux), stream_ptr()))
    return main, aux


def frames_to_memory_maps_diffused(mode, palette_rgb, rgb, weights, divisor, out=None):
    """frames_to_memory_maps by error diffusion with a chosen kernel (include/iivision.h:
    iiv_frames_to_memory_maps_diffused; csrc/iiv_diffuse.hip).  weights: 3 x 5 (or 15) integers 0..255, weights[dy][dx + 2] the
    share, in `divisor`-ths, of pixel (y + dy, k + dx); divisor 1..64.  The library refuses (IIVError, nothing launched) a
    divisor outside 1..64, a weight on the pixel itself or left of it on its row, and weights that sum to more than the
    divisor.  rgb, out and the asynchrony: exactly as frames_to_memory_maps.  The named kernels: frame_grabber.DIFFUSION_KERNELS."""
    _cuda_u8(rgb, "rgb")
    if tuple(rgb.shape[1:]) != (192, 280, 3):
        raise ValueError("rgb has shape %s, not (n, 192, 280, 3)" % (tuple(rgb.shape),))
    w = np.asarray(weights)
    if w.size != 15 or not np.issubdtype(w.dtype, np.integer) or w.min() < 0 or w.max() > 255:
        raise ValueError("weights must be 3 x 5 integers in 0..255")
    w = np.ascontiguousarray(w, dtype=np.uint8).reshape(15)
    n = int(rgb.shape[0])
    pal = np.ascontiguousarray(palette_rgb, dtype=np.uint8).reshape(48)
    main, aux = _memory_maps_out(mode, n, out)
    check(lib().iiv_frames_to_memory_maps_diffused(mode, hptr(pal), n, dptr(rgb), hptr(w), int(divisor), dptr(main), dptr(aux),
                                                   stream_ptr()))
    return main, aux


# ---- f10: direct ingest ---------------------------------------------------------------

def frames_to_memory_maps_direct(mode, palette_rgb, rgb, dither=0, cost=False, out=None):
    """rgb: CUDA uint8 (n, 192, 280 or 560, 3) -> (main, aux) CUDA uint8 (n, 32, 256), aux None for HGR: per screen row the bytes
    whose RENDERED dots are nearest the source (include/iivision.h: iiv_frames_to_memory_maps_direct).  dither: 0..255, the
    amplitude of the ordered dither added to the target (no error diffusion here).  cost=True: (main, aux, cost), cost a CUDA
    uint64 (n,) tensor of the frames' summed squared differences.  out and the asynchrony: exactly as frames_to_memory_maps."""
    torch = _torch()
    if mode not in (HGR, DHGR):
        raise ValueError("mode must be HGR or DHGR")
    _cuda_u8(rgb, "rgb")
    if rgb.dim() != 4 or int(rgb.shape[1]) != 192 or int(rgb.shape[2]) not in REF_WIDTHS or int(rgb.shape[3]) != 3:
        raise ValueError("rgb has shape %s, not (n, 192, 280 or 560, 3)" % (tuple(rgb.shape),))
    n = int(rgb.shape[0])
    pal = np.ascontiguousarray(palette_rgb, dtype=np.uint8).reshape(48)
    main, aux = _memory_maps_out(mode, n, out)
    d_cost = torch.empty((n,), dtype=torch.uint64, device="cuda") if cost else None
    if n:   # (empty tensors have no address to hand over)
        check(lib().iiv_frames_to_memory_maps_direct(mode, hptr(pal), n, dptr(rgb), int(rgb.shape[2]), int(dither), dptr(main), dptr(aux),
                                                     dptr(d_cost), stream_ptr()))
    return (main, aux, d_cost) if cost else (main, aux)


# ---- f6: mono playback mode -----------------------------------------------------------

MONO_SIZE = {HGR: (192, 280), DHGR: (192, 560)}   # (H, W) of a source frame: one pixel per dot of a monochrome screen


def frames_to_memory_maps_mono(mode, rgb, dither=0, out=None):
    """rgb: CUDA uint8 (n, 192, W, 3), W = 560 (DHGR) or 280 (HGR): one pixel per dot of a monochrome screen -> (main, aux)
    CUDA uint8 (n, 32, 256); aux is None for HGR (include/iivision.h: iiv_frames_to_memory_maps_mono).
    dither: 0..255 = amplitude of the 4x4 ordered dither, DITHER_DIFFUSION = Floyd-Steinberg over the dots.
    out=(main, aux) and the asynchrony on torch's current stream: exactly as frames_to_memory_maps."""
    if mode not in MONO_SIZE:
        raise ValueError("mode must be HGR or DHGR")
    _cuda_u8(rgb, "rgb")
    if tuple(rgb.shape[1:]) != MONO_SIZE[mode] + (3,):
        raise ValueError("rgb has shape %s, not (n, %d, %d, 3)" % ((tuple(rgb.shape),) + MONO_SIZE[mode]))
    n = int(rgb.shape[0])
    main, aux = _memory_maps_out(mode, n, out)
    check(lib().iiv_frames_to_memory_maps_mono(mode, n, dptr(rgb), int(dither), dptr(main), dptr(aux), stream_ptr()))
    return main, aux


# ---- f7: preview ----------------------------------------------------------------------

RENDER_SIZE = (192, 560)   # (H, W) of a rendered screen, both modes


def _render_out(n, out):
    """The (n, 192, 560, 3) tensor a render call writes: new, or the caller's contiguous CUDA uint8 `out` of that many bytes."""
    torch = _torch()
    if out is None:
        return torch.empty((n,) + RENDER_SIZE + (3,), dtype=torch.uint8, device="cuda")
    _cuda_u8(out, "out")
    if out.numel() != n * RENDER_SIZE[0] * RENDER_SIZE[1] * 3:
        raise ValueError("out must hold n * 192 * 560 * 3 bytes")
    return out


def render_rgb(mode, palette_rgb, main, aux=None, out=None):
    """main / aux: contiguous CUDA uint8 memory maps of n * 8192 bytes each ((n, 32, 256), or any shape that ends in (32, 256);
    aux is ignored for HGR) -> CUDA uint8 (n, 192, 560, 3): the screen through the reference's colour model (include/iivision.h:
    iiv_render_rgb).  Asynchronous on torch's current stream, as frames_to_memory_maps is."""
    if mode not in (HGR, DHGR):
        raise ValueError("mode must be HGR or DHGR")
    for t, name in ((main, "main"), (aux, "aux")) if mode == DHGR else ((main, "main"),):
        _cuda_u8(t, name)
        if t.numel() % 8192 or t.numel() != main.numel():
            raise ValueError("%s must hold n memory maps of 8192 bytes%s" % (name, "" if t is main else ", as many as main"))
    n = main.numel() // 8192
    pal = np.ascontiguousarray(palette_rgb, dtype=np.uint8).reshape(48)
    out = _render_out(n, out)
    check(lib().iiv_render_rgb(mode, hptr(pal), n, dptr(main), dptr(aux if mode == DHGR else None), dptr(out), stream_ptr()))
    return out.view((n,) + RENDER_SIZE + (3,))


def encoder_render(encoder, palette_rgb, first_stream=0, n_streams=None, out=None):
    """The screens the streams first_stream .. of an Encoder hold right now (behind the launches already on torch's current
    stream) -> CUDA uint8 (n_streams, 192, 560, 3), rendered from the encoder's own device state (iiv_encoder_render)."""
    n = encoder.n_streams - int(first_stream) if n_streams is None else int(n_streams)
    if first_stream < 0 or n < 0 or first_stream + n > encoder.n_streams:
        raise ValueError("streams %d .. %d of an encoder of %d" % (first_stream, first_stream + n - 1, encoder.n_streams))
    pal = np.ascontiguousarray(palette_rgb, dtype=np.uint8).reshape(48)
    out = _render_out(n, out)
    check(lib().iiv_encoder_render(encoder._h, int(first_stream), n, hptr(pal), dptr(out), stream_ptr()))
    return out.view((n,) + RENDER_SIZE + (3,))


# ---- f8: screen error -----------------------------------------------------------------

REF_WIDTHS = (280, 560)    # a reference picture has one pixel per two dots or one per dot


def _error_args(n, ref, out):
    """Checks the reference (n, 192, 280 or 560, 3) and the (n, 3, 3) uint64 tensor an error call writes (new, or the caller's
    contiguous CUDA `out` of 8-byte elements and that many bytes) -> (ref_width, out)."""
    torch = _torch()
    _cuda_u8(ref, "ref")
    if ref.dim() != 4 or int(ref.shape[0]) != n or int(ref.shape[1]) != 192 or int(ref.shape[2]) not in REF_WIDTHS or int(ref.shape[3]) != 3:
        raise ValueError("ref has shape %s, not (%d, 192, 280 or 560, 3)" % (tuple(ref.shape), n))
    if out is None:
        return int(ref.shape[2]), torch.empty((n, 3, 3), dtype=torch.uint64, device="cuda")
    if not out.is_cuda or not out.is_contiguous() or out.element_size() != 8 or out.numel() != n * 9:
        raise ValueError("out must be a contiguous CUDA tensor of n * 9 eight-byte integers")
    return int(ref.shape[2]), out


def render_error(mode, palette_rgb, main, aux, ref, out=None):
    """main / aux: memory maps as render_rgb takes them; ref: contiguous CUDA uint8 (n, 192, W, 3), W = 560 (one pixel per dot)
    or 280 (one per two dots) -> CUDA uint64 (n, 3, 3), [frame][level][channel]: the exact sums of squared differences between
    the screen render_rgb would draw and ref, per dot (level 0), per quad of four dots (1) and per unit of sixteen (2)
    (include/iivision.h: iiv_render_error).  The rendering never leaves the chip.  Asynchronous on torch's current stream."""
    if mode not in (HGR, DHGR):
        raise ValueError("mode must be HGR or DHGR")
    for t, name in ((main, "main"), (aux, "aux")) if mode == DHGR else ((main, "main"),):
        _cuda_u8(t, name)
        if t.numel() % 8192 or t.numel() != main.numel():
            raise ValueError("%s must hold n memory maps of 8192 bytes%s" % (name, "" if t is main else ", as many as main"))
    n = main.numel() // 8192
    pal = np.ascontiguousarray(palette_rgb, dtype=np.uint8).reshape(48)
    width, out = _error_args(n, ref, out)
    if n == 0:   # (nothing to measure, nothing written: empty tensors have no address to hand over)
        return out.view((0, 3, 3))
    check(lib().iiv_render_error(mode, hptr(pal), n, dptr(main), dptr(aux if mode == DHGR else None), dptr(ref), width, dptr(out),
                                 stream_ptr()))
    return out.view((n, 3, 3))


def encoder_render_error(encoder, palette_rgb, ref, first_stream=0, n_streams=None, out=None):
    """The same sums for the screens the streams first_stream .. of an Encoder hold right now (behind the launches already on
    torch's current stream), measured on the encoder's own device state (iiv_encoder_render_error): ref[i] belongs to stream
    first_stream + i -> CUDA uint64 (n_streams, 3, 3)."""
    n = encoder.n_streams - int(first_stream) if n_streams is None else int(n_streams)
    if first_stream < 0 or n < 0 or first_stream + n > encoder.n_streams:
        raise ValueError("streams %d .. %d of an encoder of %d" % (first_stream, first_stream + n - 1, encoder.n_streams))
    pal = np.ascontiguousarray(palette_rgb, dtype=np.uint8).reshape(48)
    width, out = _error_args(n, ref, out)
    if n == 0:
        return out.view((0, 3, 3))
    check(lib().iiv_encoder_render_error(encoder._h, int(first_stream), n, hptr(pal), dptr(ref), width, dptr(out), stream_ptr()))
    return out.view((n, 3, 3))


# ---- f9: reading an opcode stream -------------------------------------------------------

A2M_STATUS = ("OK", "BAD_LENGTH", "BAD_HEADER", "BAD_ACK", "BAD_ADDRESS", "NO_TERMINATE", "BAD_PADDING")   # IIV_A2M_*
A2M_OK = 0


def a2m_max_ops(length):
    """Whole opcode slots in a stream of that many bytes (iiv_a2m_max_ops).  Host only."""
    return int(lib().iiv_a2m_max_ops(int(length)))


class A2mReaderHandle:
    """An iiv_a2m_reader: the device copy of the address table the reading kernels look opcodes up in.  Creation raises
    IIVError(ERR_INVALID), before the device is touched, unless the 1024 tick addresses, ack and terminate are pairwise distinct."""

    def __init__(self, tick_addr, ack_addr, terminate_addr):
        ta = np.ascontiguousarray(tick_addr, dtype=np.uint16).reshape(1024)
        h = C.c_void_p()
        check(lib().iiv_a2m_reader_create(hptr(ta), int(ack_addr), int(terminate_addr), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().iiv_a2m_reader_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _batch(data):
        _cuda_u8(data, "data")
        if data.dim() != 2 or int(data.shape[1]) < 2048:
            raise ValueError("data has shape %s, not (n_streams, stride >= 2048)" % (tuple(data.shape),))
        return int(data.shape[0]), int(data.shape[1])

    @staticmethod
    def _info(info, n):
        torch = _torch()
        if not (isinstance(info, torch.Tensor) and info.is_cuda and info.dtype == torch.int64 and info.is_contiguous()
                and tuple(info.shape) == (n, 4)):
            raise ValueError("info must be a contiguous CUDA int64 tensor (%d, 4), as scan returns it" % n)

    def scan(self, data, lengths):
        """data: CUDA uint8 (S, stride); lengths: CUDA int64 (S,) -> CUDA int64 (S, 4) {status, mode, n_ops, position}.
        Asynchronous on torch's current stream."""
        torch = _torch()
        S, stride = self._batch(data)
        if not (isinstance(lengths, torch.Tensor) and lengths.is_cuda and lengths.dtype == torch.int64 and lengths.is_contiguous()
                and tuple(lengths.shape) == (S,)):
            raise ValueError("lengths must be a contiguous CUDA int64 tensor (%d,)" % S)
        info = torch.empty((S, 4), dtype=torch.int64, device="cuda")
        if S:
            check(lib().iiv_a2m_scan(self._h, S, dptr(data), stride, dptr(lengths), dptr(info), stream_ptr()))
        return info

    def decode(self, data, info):
        """-> CUDA uint8 ops (S, max_ops, 6), ticks (S, max_ops), banks (S, max_ops), max_ops = a2m_max_ops(stride); row s is
        written up to info[s, 2] and zero behind it.  Asynchronous."""
        torch = _torch()
        S, stride = self._batch(data)
        self._info(info, S)
        n = a2m_max_ops(stride)
        ops = torch.zeros((S, n, 6), dtype=torch.uint8, device="cuda")
        ticks = torch.zeros((S, n), dtype=torch.uint8, device="cuda")
        banks = torch.zeros((S, n), dtype=torch.uint8, device="cuda")
        if S:
            check(lib().iiv_a2m_decode(self._h, S, dptr(data), stride, dptr(info), dptr(ops), n * 6, dptr(ticks), dptr(banks), n,
                                       stream_ptr()))
        return ops, ticks, banks

    def replay(self, data, info, first, every, n, init=None):
        """-> (main, aux) CUDA uint8 (S, n, 32, 256): snapshot j after the first min(first + j * every, n_ops) opcodes.
        init: (main, aux) contiguous CUDA uint8 (S, 32, 256) starting state, None = zeros.  Asynchronous."""
        torch = _torch()
        S, stride = self._batch(data)
        self._info(info, S)
        first, every, n = int(first), int(every), int(n)
        if first < 0 or every < 1 or n < 1:
            raise ValueError("replay: first >= 0, every >= 1, n >= 1")
        im = ia = None
        if init is not None:
            im, ia = init
            for t in (im, ia):
                _cuda_u8(t, "each init tensor")
                if t.numel() != S * 8192:
                    raise ValueError("each init tensor must hold n_streams * 8192 bytes")
        main = torch.empty((S, n, 32, 256), dtype=torch.uint8, device="cuda")
        aux = torch.empty((S, n, 32, 256), dtype=torch.uint8, device="cuda")
        if S:
            check(lib().iiv_a2m_replay(self._h, S, dptr(data), stride, dptr(info), min(first, 2 ** 62), min(every, 2 ** 62), n,
                                       dptr(im), dptr(ia), dptr(main), dptr(aux), stream_ptr()))
        return main, aux


# ---- f13: speaker preview -------------------------------------------------------------

SPEAKER_DECIM, SPEAKER_ORDER, SPEAKER_GAIN = 23, 3, 16384   # the defaults of every speaker_pcm: 1020484 / 23 = 44 369 Hz


def speaker_periods(n_ops):
    """73-cycle periods a stream of n_ops opcodes plays: the opcodes and two per ACK (iiv_speaker_periods).  Host only."""
    return int(lib().iiv_speaker_periods(int(n_ops)))


def speaker_sample_count(n_ops, decim=SPEAKER_DECIM):
    """PCM samples of a stream of n_ops opcodes at one sample per `decim` cycles (iiv_speaker_sample_count).  Host only."""
    n = lib().iiv_speaker_sample_count(int(n_ops), int(decim))
    if n < 0:
        check(int(n))
    return int(n)


def speaker_pcm(ticks, counts=None, decim=SPEAKER_DECIM, order=SPEAKER_ORDER, gain=SPEAKER_GAIN, out=None, d_err=None):
    """What the ticks of S streams sound like: ticks CUDA uint8 (S, n) with contiguous rows (audio_ticks' or A2mReaderHandle.decode's
    output) -> (CUDA int16 (S, pcm_stride), int64 numpy sample counts M(s)); row s is written up to M(s) and left as it was -- zero
    in a new tensor -- behind it (include/iivision.h: iiv_speaker_pcm).  counts: the opcode count of every stream, None = n for all;
    a sequence or numpy array, or a CUDA int64 tensor that is handed over as it is -- a scan's info[:, 2] view, stride 4,
    included -- and then costs the one device-to-host copy that the returned counts need.  out: a CUDA int16 (S, >=
    speaker_sample_count(n, decim)) tensor with contiguous rows.  d_err: a CUDA int32 tensor of one element that is set to 1 if a
    tick byte is not an even number in 4..66 (never cleared).  Asynchronous on torch's current stream."""
    torch = _torch()
    if not (isinstance(ticks, torch.Tensor) and ticks.is_cuda and ticks.dtype == torch.uint8 and ticks.dim() == 2
            and (ticks.shape[1] == 0 or ticks.stride(1) == 1)):
        raise ValueError("ticks must be a CUDA uint8 tensor (n_streams, n) with contiguous rows")
    S, n = int(ticks.shape[0]), int(ticks.shape[1])
    if S > 1 and int(ticks.stride(0)) != n:   # (the C ABI takes the row stride as the bound of every count)
        ticks = ticks.contiguous()
    if isinstance(counts, torch.Tensor):
        if not (counts.is_cuda and counts.dtype == torch.int64 and counts.dim() == 1 and int(counts.shape[0]) == S):
            raise ValueError("counts must be a CUDA int64 tensor (%d,)" % S)
        d_counts, host = counts, None
    else:
        host = np.ascontiguousarray(np.broadcast_to(np.asarray(n if counts is None else counts, dtype=np.int64), (S,)))
        d_counts = torch.from_numpy(host.copy()).cuda()
    if not (1 <= int(decim) <= 73 and 1 <= int(order) <= 4 and 0 <= int(gain) <= 32767):
        raise ValueError("speaker_pcm: decim 1..73, order 1..4, gain 0..32767")
    width = speaker_sample_count(n, decim)
    if out is None:
        out = torch.zeros((S, max(-(-width // 8) * 8, 8)), dtype=torch.int16, device="cuda")   # rows start 16-byte aligned
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int16 and out.dim() == 2 and int(out.shape[0]) == S
              and int(out.shape[1]) >= width and out.stride(1) == 1):
        raise ValueError("out must be a CUDA int16 tensor (n_streams, >= %d) with contiguous rows" % width)
    if d_err is not None and not (isinstance(d_err, torch.Tensor) and d_err.is_cuda and d_err.dtype == torch.int32 and d_err.numel() == 1):
        raise ValueError("d_err must be a CUDA int32 tensor of one element")
    if S and n:
        check(lib().iiv_speaker_pcm(S, dptr(ticks), n, dptr(d_counts),
                                    int(d_counts.stride(0)) if S > 1 else 1, int(decim), int(order), int(gain), dptr(out),
                                    int(out.stride(0)) if S > 1 else int(out.shape[1]), dptr(d_err), stream_ptr()))
    if host is None:
        host = d_counts.cpu().numpy()   # (behind the launch: nothing waits for the host in front of the kernel)
    return out, np.array([speaker_sample_count(c, decim) for c in np.clip(host, 0, n)], dtype=np.int64)


# ---- clip stages (f14, f15): the frames of a clip and the out= argument -------------------

def _stride(t, dim, default):
    """t.stride(dim) where it means something: a dimension of one element has no stride of its own"""
    return int(t.stride(dim)) if int(t.shape[dim]) > 1 else default


def _dense_frames(t, name):
    """ValueError unless the last three dimensions of t are one dense (H, W, 3) frame"""
    if not (int(t.shape[-1]) == 3 and _stride(t, -1, 1) == 1 and _stride(t, -2, 3) == 3
            and _stride(t, -3, 3 * int(t.shape[-2])) == 3 * int(t.shape[-2])):
        raise ValueError("%s: a frame must be dense (H, W, 3) bytes" % name)


def _clip_frames(frames, name):
    """(c, n, H, W, clip stride, frame stride, several) of a CUDA uint8 tensor (n, H, W, 3) or (c, n, H, W, 3) with dense frames of
    a positive multiple of 4 pixels"""
    torch = _torch()
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() in (4, 5)):
        raise ValueError("%s must be a CUDA uint8 tensor (n, H, W, 3) or (c, n, H, W, 3)" % name)
    _dense_frames(frames, name)
    several = frames.dim() == 5
    c = int(frames.shape[0]) if several else 1
    n, H, W = (int(v) for v in frames.shape[-4:-1])
    if H * W <= 0 or (H * W) % 4:
        raise ValueError("a frame must hold a positive multiple of 4 pixels, got %d x %d" % (H, W))
    frame = _stride(frames, -4, H * W * 3)
    return c, n, H, W, (_stride(frames, 0, n * frame) if several else n * frame), frame, several


def _clip_out(out, frames):
    """(out, clip stride, frame stride) of a clip stage's out= argument: None is a new contiguous tensor of the checked frames' shape
    on their device, anything else a CUDA uint8 tensor of exactly that shape with dense frames (frames itself: in place)"""
    if out is None:
        out = _torch().empty(tuple(frames.shape), dtype=frames.dtype, device=frames.device)
    clip_stride, frame_stride = _clip_frames(out, "out")[4:6]
    if tuple(out.shape) != tuple(frames.shape):
        raise ValueError("out must be a CUDA uint8 tensor of frames' shape %s" % (tuple(frames.shape),))
    return out, clip_stride, frame_stride


# ---- f14: temporal hold ---------------------------------------------------------------

def temporal_pair(temporal):
    """(lo, hi) of a temporal hold as two ints; ValueError unless 0 <= lo <= hi <= 255 (include/iivision.h f14)."""
    try:
        lo, hi = temporal
        if int(lo) != lo or int(hi) != hi:
            raise ValueError
        lo, hi = int(lo), int(hi)
    except (TypeError, ValueError):
        raise ValueError("a temporal hold is two integers (lo, hi), got %r" % (temporal,)) from None
    if not 0 <= lo <= hi <= 255:
        raise ValueError("a temporal hold needs 0 <= lo <= hi <= 255, got (%d, %d)" % (lo, hi))
    return lo, hi


def temporal_hold(frames, lo, hi, state=None, out=None, counts=False):
    """The temporal hold along the frames of a clip (include/iivision.h: iiv_temporal_hold): a pixel within `lo` of its held value
    keeps the held bytes, one more than `hi` away takes the source's, one between moves part of the way.  frames: CUDA uint8
    (n, H, W, 3) for one clip or (c, n, H, W, 3) for several; frame and clip strides are free (multiples of 4 bytes), a frame is
    dense, H * W a multiple of 4.  state: None starts the hold at frame 0 (`first`) and allocates the held frames; the state an
    earlier call returned -- contiguous CUDA uint8 (H, W, 3) or (c, H, W, 3) -- continues that clip and is updated in place.
    out: a tensor of frames' shape to write into (frames itself: in place), by default a new contiguous one.
    -> (out, state), or (out, state, counts) with counts=True: CUDA int32 (n, 3) or (c, n, 3), the pixels held, blended and passed
    of every frame.  Asynchronous on torch's current stream, like resize_frames."""
    torch = _torch()
    lo, hi = temporal_pair((lo, hi))
    c, n, H, W, clip_stride, frame_stride, several = _clip_frames(frames, "frames")
    out, out_clip_stride, out_frame_stride = _clip_out(out, frames)
    state_shape = ((c,) if several else ()) + (H, W, 3)
    first = state is None
    if first:
        state = torch.empty(state_shape, dtype=torch.uint8, device=frames.device)
    else:
        _cuda_u8(state, "state")
        if tuple(state.shape) != state_shape:
            raise ValueError("state has shape %s, these frames need %s" % (tuple(state.shape), state_shape))
    d_counts = torch.empty(((c,) if several else ()) + (n, 3), dtype=torch.int32, device=frames.device) if counts else None
    with torch.cuda.device(frames.device):
        check(lib().iiv_temporal_hold(c, n, H * W, dptr(frames), clip_stride, frame_stride, dptr(out), out_clip_stride, out_frame_stride,
                                      dptr(state), H * W * 3, 1 if first else 0, lo, hi, dptr(d_counts), stream_ptr()))
    return (out, state, d_counts) if counts else (out, state)


# ---- f15: picture levels ---------------------------------------------------------------

LEVELS_PPM = (5000, 5000)     # the 0.5th and 99.5th percentiles, as the reference's audio normalisation takes them (audio.py:60-78)
LEVELS_MATRIX_RANGE = (-2048, 2047)   # Q8 entries of the 3 x 3 matrix: +-8.0 (include/iivision.h f15)


def levels_histogram(frames):
    """The histograms of every frame (include/iivision.h: iiv_levels_histogram).  frames: CUDA uint8 (n, H, W, 3) for one clip or
    (c, n, H, W, 3) for several; frame and clip strides are free (multiples of 4 bytes), a frame is dense, H * W a multiple of 4.
    -> CUDA int32 (n, 4, 256) or (c, n, 4, 256): per frame the counts of R, G, B and Y = (77 R + 150 G + 29 B + 128) >> 8 (the
    bits of a uint32: a frame of 2^31 equal pixels reads as negative).  Asynchronous on torch's current stream."""
    torch = _torch()
    c, n, H, W, clip_stride, frame_stride, several = _clip_frames(frames, "frames")
    hist = torch.empty(((c,) if several else ()) + (n, 4, 256), dtype=torch.int32, device=frames.device)
    with torch.cuda.device(frames.device):
        check(lib().iiv_levels_histogram(c, n, H * W, dptr(frames), clip_stride, frame_stride, dptr(hist), stream_ptr()))
    return hist


def levels_auto(hist256, lo_ppm=LEVELS_PPM[0], hi_ppm=LEVELS_PPM[1]):
    """(black, white) from one histogram of 256 counts (include/iivision.h: iiv_levels_auto): at most lo_ppm millionths of the
    pixels lie below black and hi_ppm above white; an empty histogram, or points that meet, give (0, 255).  Host only."""
    h = np.asarray(hist256)
    if h.shape != (256,) or h.dtype.kind not in "iu" or (h.dtype.kind == "i" and h.size and int(h.min()) < 0):
        raise ValueError("hist256 must be 256 non-negative integer counts")
    if not (0 <= int(lo_ppm) <= 500000 and 0 <= int(hi_ppm) <= 500000 and int(lo_ppm) == lo_ppm and int(hi_ppm) == hi_ppm):
        raise ValueError("lo_ppm and hi_ppm are integers in 0..500000, got (%r, %r)" % (lo_ppm, hi_ppm))
    h = np.ascontiguousarray(h, dtype=np.uint64)
    black, white = C.c_int(0), C.c_int(255)
    check(lib().iiv_levels_auto(hptr(h), int(lo_ppm), int(hi_ppm), C.byref(black), C.byref(white)))
    return black.value, white.value


def levels_tables(lut, matrix, c):
    """The tables of levels_apply as the C ABI takes them, on the host: (uint8 (k, 3, 256), int16 (k, 10), lut_stride,
    matrix_stride) for c clips.  lut: uint8 (256,) -- one table for the three channels --, (3, 256), or (c, 3, 256) per clip;
    matrix: None (256 * I), (3, 3) or (c, 3, 3) integers in -2048..2047, checked here because the library cannot.  A matrix row
    is 18 bytes padded to 20."""
    lut = np.asarray(lut)
    if lut.dtype != np.uint8 or lut.shape not in ((256,), (3, 256), (c, 3, 256)):
        raise ValueError("lut must be uint8 (256,), (3, 256) or (%d, 3, 256), got %s %s" % (c, lut.dtype, lut.shape))
    lut_stride = 768 if lut.ndim == 3 else 0
    lut = np.ascontiguousarray(np.broadcast_to(lut, (3, 256)) if lut.ndim < 3 else lut).reshape(-1, 3, 256)
    m = np.asarray(256 * np.eye(3, dtype=np.int64) if matrix is None else matrix)
    if m.dtype.kind not in "iu" or m.shape not in ((3, 3), (c, 3, 3)):
        raise ValueError("matrix must be integers (3, 3) or (%d, 3, 3), got %s %s" % (c, m.dtype, m.shape))
    if m.size and not (LEVELS_MATRIX_RANGE[0] <= int(m.min()) and int(m.max()) <= LEVELS_MATRIX_RANGE[1]):
        raise ValueError("matrix entries are Q8 in %d..%d" % LEVELS_MATRIX_RANGE)
    matrix_stride = 20 if m.ndim == 3 else 0
    padded = np.zeros((m.size // 9, 10), np.int16)
    padded[:, :9] = m.reshape(-1, 9)
    return lut, padded, lut_stride, matrix_stride


def levels_apply(frames, lut, matrix=None, out=None):
    """A table per channel and a 3 x 3 matrix behind it, on every pixel (include/iivision.h: iiv_levels_apply): a_c = lut[c][x_c],
    y_c = clamp((m[c] . a + 128) >> 8, 0, 255).  frames: as levels_histogram's.  lut, matrix: host arrays, see levels_tables (one
    for all clips, or one per clip).  out: a tensor of frames' shape to write into (frames itself: in place), by default a new
    contiguous one.  -> out.  Asynchronous on torch's current stream (the tables are uploaded on it)."""
    torch = _torch()
    c, n, H, W, clip_stride, frame_stride, several = _clip_frames(frames, "frames")
    out, out_clip_stride, out_frame_stride = _clip_out(out, frames)
    lut, m, lut_stride, matrix_stride = levels_tables(lut, matrix, c)
    with torch.cuda.device(frames.device):
        d_lut, d_m = torch.from_numpy(lut.copy()).to(frames.device), torch.from_numpy(m).to(frames.device)
        check(lib().iiv_levels_apply(c, n, H * W, dptr(frames), clip_stride, frame_stride, dptr(out), out_clip_stride, out_frame_stride,
                                     dptr(d_lut), lut_stride, dptr(d_m), matrix_stride, stream_ptr()))
    return out


# ---- f16: spatial filter ---------------------------------------------------------------

FILTER_GAIN_RANGE = (-256, 1024)   # Q8 entries of the gain table (include/iivision.h f16)
FILTER_SIZE_MAX = 4096             # rows and pixels of a row


def filter_tables(taps_x, taps_y, gain):
    """(uint16 (5,), uint16 (5,), int16 (256,)) as the C ABI takes them; ValueError unless each tap set is five integers in 0..256
    that sum to 256 and gain is 256 integers in -256..1024 (include/iivision.h f16)."""
    taps = []
    for name, t in (("taps_x", taps_x), ("taps_y", taps_y)):
        a = np.asarray(t)
        if a.shape != (5,) or a.dtype.kind not in "iu":
            raise ValueError("%s must be five integers, got %r" % (name, t))
        a = a.astype(np.int64)
        if int(a.min()) < 0 or int(a.max()) > 256 or int(a.sum()) != 256:
            raise ValueError("%s must be five taps in 0..256 that sum to 256, got %s" % (name, a.tolist()))
        taps.append(np.ascontiguousarray(a, dtype=np.uint16))
    g = np.asarray(gain)
    if g.shape != (256,) or g.dtype.kind not in "iu":
        raise ValueError("gain must be 256 integers, got %s %s" % (g.dtype, g.shape))
    g = g.astype(np.int64)
    if int(g.min()) < FILTER_GAIN_RANGE[0] or int(g.max()) > FILTER_GAIN_RANGE[1]:
        raise ValueError("gain entries are Q8 in %d..%d" % FILTER_GAIN_RANGE)
    return taps[0], taps[1], np.ascontiguousarray(g, dtype=np.int16)


def filter_frames(frames, taps_x, taps_y, gain, out=None):
    """The spatial filter on every frame (include/iivision.h: iiv_filter_frames): B the separable 5 x 5 blur of the frame under
    taps_x and taps_y (edges replicated), d = p - B, m the largest |d| of the pixel's channels, y_c = clamp(p_c + ((gain[m] d_c +
    128) >> 8)).  frames: CUDA uint8 (n, H, W, 3) for one clip or (c, n, H, W, 3) for several; frame and clip strides are free
    (multiples of 4 bytes), a frame is dense, H is 1..4096 and W a multiple of 4 in 4..4096.  taps_x, taps_y, gain: see
    filter_tables.  out: a tensor of frames' shape to write into, by default a new contiguous one; it must not share storage with
    frames (a neighbour's source would be overwritten).  -> out.  Asynchronous on torch's current stream."""
    torch = _torch()
    tx, ty, g = filter_tables(taps_x, taps_y, gain)
    c, n, H, W, clip_stride, frame_stride, several = _clip_frames(frames, "frames")
    if not (1 <= H <= FILTER_SIZE_MAX and 4 <= W <= FILTER_SIZE_MAX and W % 4 == 0):
        raise ValueError("a filtered frame has 1..%d rows of a multiple of 4 in 4..%d pixels, got %d x %d"
                         % (FILTER_SIZE_MAX, FILTER_SIZE_MAX, H, W))
    if out is not None and isinstance(out, torch.Tensor) and out.is_cuda and out.device == frames.device \
            and out.untyped_storage().data_ptr() == frames.untyped_storage().data_ptr():
        raise ValueError("out must not share storage with frames: the filter reads a pixel's neighbours")
    out, out_clip_stride, out_frame_stride = _clip_out(out, frames)
    with torch.cuda.device(frames.device):
        check(lib().iiv_filter_frames(c, n, H, W, dptr(frames), clip_stride, frame_stride, dptr(out), out_clip_stride, out_frame_stride,
                                      hptr(tx), hptr(ty), hptr(g), stream_ptr()))
    return out


# ---- f4: the audio track ------------------------------------------------------------

AUDIO_BITRATE = 14700          # audio.Audio(bitrate=14700) (audio.py:35)
AUDIO_BLOCK_FRAMES = 128 * 1024  # audio.py:98 f.read_data(128 * 1024): frames per decode block


def audio_tick_count(n_frames, rate, bitrate=AUDIO_BITRATE, block_frames=AUDIO_BLOCK_FRAMES):
    """Ticks (= opcodes) of one stream of n_frames frames at `rate` Hz.  Host only."""
    n = lib().iiv_audio_tick_count(int(n_frames), int(rate), int(bitrate), int(block_frames))
    if n < 0:
        check(int(n))
    return int(n)


def _audio_streams(pcm, n_frames, channels, rate):
    """pcm: CUDA int16 (S, stride) (each row interleaved frames); per-stream frame counts / channels / rates (scalars
    broadcast) -> the host arrays of the C ABI."""
    torch = _torch()
    if not (pcm.is_cuda and pcm.dtype == torch.int16 and pcm.dim() == 2 and pcm.stride(1) == 1):
        raise ValueError("pcm must be a CUDA int16 tensor (n_streams, samples) with contiguous rows")
    S = int(pcm.shape[0])
    nf = np.ascontiguousarray(np.broadcast_to(np.asarray(n_frames, dtype=np.int64), (S,)), dtype=C.c_long)
    ch = np.ascontiguousarray(np.broadcast_to(np.asarray(channels, dtype=np.int32), (S,)), dtype=np.int32)
    rt = np.ascontiguousarray(np.broadcast_to(np.asarray(rate, dtype=np.int32), (S,)), dtype=np.int32)
    if S and int((nf.astype(np.int64) * ch).max()) > int(pcm.shape[1]):   # (the C side can only check the row stride)
        raise ValueError("pcm rows hold %d samples; a stream needs n_frames * channels = %d" % (
            int(pcm.shape[1]), int((nf.astype(np.int64) * ch).max())))
    return S, nf, ch, rt


AUDIO_PREFIX_BYTES = 10 * 1024 * 1024   # audio.py:63 _normalization(read_bytes=1024 * 1024 * 10)
AUDIO_RAW_BLOCK_FRAMES = 1024           # audioread's wave backend: read_data() reads 1024 frames a block


def audio_prefix_frames(n_frames, channels):
    """The frames Audio._normalization decodes (audio.py:62-66: reads until more than 10 MiB are held); the rule
    iiv_audio_normalization applies."""
    blocks = AUDIO_PREFIX_BYTES // (AUDIO_RAW_BLOCK_FRAMES * 2 * int(channels)) + 1
    return min(int(n_frames), blocks * AUDIO_RAW_BLOCK_FRAMES)


def audio_ticks(pcm, n_frames, channels, rate, normalization, bitrate=AUDIO_BITRATE, block_frames=AUDIO_BLOCK_FRAMES,
                out=None):
    """Speaker duty cycles (4..66, even) of S streams: pcm CUDA int16 (S, >= n_frames * channels) -> (CUDA uint8
    (S, max tick count) -- bytes past a stream's own count are left as they were --, int64 numpy tick counts).
    normalization: per stream (or one value).  out: a CUDA uint8 (S, >= max count) tensor with contiguous rows to write into.
    Asynchronous on torch's current stream."""
    torch = _torch()
    S, nf, ch, rt = _audio_streams(pcm, n_frames, channels, rate)
    nm = np.ascontiguousarray(np.broadcast_to(np.asarray(normalization, dtype=np.float64), (S,)))
    counts = np.array([audio_tick_count(nf[s], rt[s], bitrate, block_frames) for s in range(S)], dtype=C.c_long)
    width = int(counts.max()) if S else 0
    if out is None:
        out = torch.zeros((S, max(width, 1)), dtype=torch.uint8, device="cuda")
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == S and out.shape[1] >= width
              and out.stride(1) == 1):
        raise ValueError("out must be a CUDA uint8 tensor (n_streams, >= %d) with contiguous rows" % width)
    got = np.zeros(S, dtype=C.c_long)
    check(lib().iiv_audio_ticks(S, dptr(pcm), int(pcm.stride(0)), hptr(nf), hptr(ch), hptr(rt), int(bitrate),
                                int(block_frames), hptr(nm), dptr(out), int(out.stride(0)), hptr(got), stream_ptr()))
    return out, got.astype(np.int64)


def audio_resample(pcm, n_frames, channels, rate, bitrate=AUDIO_BITRATE):
    """audio.Audio._decode of each whole stream as one block -> (CUDA float32 (S, max length), int64 numpy lengths)."""
    torch = _torch()
    S, nf, ch, rt = _audio_streams(pcm, n_frames, channels, rate)
    lens = np.array([audio_tick_count(nf[s], rt[s], bitrate, max(int(nf[s]), 1)) for s in range(S)], dtype=C.c_long)
    out = torch.zeros((S, max(int(lens.max()) if S else 0, 1)), dtype=torch.float32, device="cuda")
    got = np.zeros(S, dtype=C.c_long)
    check(lib().iiv_audio_resample(S, dptr(pcm), int(pcm.stride(0)), hptr(nf), hptr(ch), hptr(rt), int(bitrate),
                                   dptr(out), int(out.stride(0)), hptr(got), stream_ptr()))
    return out, got.astype(np.int64)


def audio_normalization(pcm, n_frames, channels, rate, bitrate=AUDIO_BITRATE):
    """audio.Audio._normalization of S streams on the device -> float64 numpy (S,) (inf for a silent prefix).
    Synchronises."""
    _torch()
    S, nf, ch, rt = _audio_streams(pcm, n_frames, channels, rate)
    out = np.zeros(S, dtype=np.float64)
    check(lib().iiv_audio_normalization(S, dptr(pcm), int(pcm.stride(0)), hptr(nf), hptr(ch), hptr(rt), int(bitrate),
                                        hptr(out), stream_ptr()))
    return out


# ---- f5: the resize -----------------------------------------------------------------

RESIZE_SIZE = (192, 280)   # (H, W): frame_grabber.py:75,100 resize((280, 192), resample=Image.LANCZOS)


def resize_coeffs(in_size, out_size):
    """The Lanczos coefficient table of one axis, in_size -> out_size samples, as Pillow builds it.  Host only ->
    (bounds int32 (out, 2) = (first input sample, taps used), coefficients int32 (out, ksize) in 22-bit fixed point)."""
    ks = C.c_int(0)
    check(lib().iiv_resize_coeffs(int(in_size), int(out_size), C.byref(ks), None, None))
    bounds = np.zeros((int(out_size), 2), np.int32)
    k = np.zeros((int(out_size), ks.value), np.int32)
    check(lib().iiv_resize_coeffs(int(in_size), int(out_size), C.byref(ks), hptr(bounds), hptr(k)))
    return bounds, k


def resize_coeffs_box(in_size, in0, in1, out_size):
    """resize_coeffs for the box [in0, in1) of an axis of in_size samples, as Pillow's Image.resize(box=) builds it
    (include/iivision.h f12): in0 and in1 are rounded to float32 first.  Host only -> (bounds, coefficients)."""
    box = np.array([in0, in1], np.float32)
    ks = C.c_int(0)
    check(lib().iiv_resize_coeffs_box(int(in_size), hptr(box), int(out_size), C.byref(ks), None, None))
    bounds = np.zeros((int(out_size), 2), np.int32)
    k = np.zeros((int(out_size), ks.value), np.int32)
    check(lib().iiv_resize_coeffs_box(int(in_size), hptr(box), int(out_size), C.byref(ks), hptr(bounds), hptr(k)))
    return bounds, k


def fit_args(h, w, H, W, box=None, rect=None, fill=(0, 0, 0)):
    """The three keywords of resize_frames / resize_frames_yuv420 as the C ABI takes them (include/iivision.h f12): None when
    all three are at their defaults (the plain entry points), else (box float32 (4,), rect int32 (4,), fill r | g << 8 | b << 16)
    with box = None the whole h x w frame and rect = None the whole H x W destination.  ValueError for a malformed keyword, a
    box that is not 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h as float32, or a rect that is not inside the destination."""
    try:
        f = tuple(int(c) for c in fill)
        if len(f) != 3 or any(c < 0 or c > 255 or c != v for c, v in zip(f, fill)):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("fill is three integers 0..255 (r, g, b), got %r" % (fill,)) from None
    if box is None and rect is None and f == (0, 0, 0):
        return None
    try:
        b = np.array((0, 0, w, h) if box is None else box, dtype=np.float32)
        if b.shape != (4,) or not np.isfinite(b).all():
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("box is four finite numbers (x0, y0, x1, y1), got %r" % (box,)) from None
    if not (0 <= b[0] < b[2] <= w and 0 <= b[1] < b[3] <= h):
        raise ValueError("box %s needs 0 <= x0 < x1 <= %d and 0 <= y0 < y1 <= %d (as float32)" % (tuple(float(v) for v in b), w, h))
    try:
        r = tuple(int(v) for v in ((0, 0, W, H) if rect is None else rect))
        if len(r) != 4 or any(v != q for v, q in zip(r, (0, 0, W, H) if rect is None else rect)):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("rect is four integers (rx, ry, rw, rh), got %r" % (rect,)) from None
    if r[0] < 0 or r[1] < 0 or r[2] < 1 or r[3] < 1 or r[0] + r[2] > W or r[1] + r[3] > H:
        raise ValueError("rect %s must lie inside the %dx%d destination with rw, rh >= 1" % (r, W, H))
    return b, np.array(r, np.int32), f[0] | f[1] << 8 | f[2] << 16


def resize_frames(rgb, size=RESIZE_SIZE, out=None, box=None, rect=None, fill=(0, 0, 0)):
    """Image.resize((W, H), LANCZOS) of every frame, byte-exact: rgb CUDA uint8 (n, h, w, 3) with unit channel stride and
    pixel stride 3 (any frame and row strides: a crop or a letterbox cut is passed as a view) -> CUDA uint8 (n, H, W, 3).
    out: a contiguous CUDA uint8 tensor of n * H * W * 3 bytes to write into.  Asynchronous on torch's current stream once a
    size pair has been used on the device (the first call with it uploads its coefficient tables and synchronises); `rgb`
    and `out` must stay alive and untouched until that stream has reached this call (as for frames_to_memory_maps).
    box, rect, fill (include/iivision.h f12, fit_args): the box (x0, y0, x1, y1) of each frame, in source pixels, is resized as
    Image.resize((rw, rh), LANCZOS, box=box) into the rectangle rect = (rx, ry, rw, rh) of the destination, and the rest of the
    destination is the colour fill = (r, g, b); all three at their defaults is the plain iiv_resize_frames."""
    torch = _torch()
    H, W = (int(v) for v in size)
    if not (rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.dim() == 4 and rgb.shape[3] == 3 and rgb.stride(3) == 1
            and rgb.stride(2) == 3):
        raise ValueError("rgb must be a CUDA uint8 tensor (n, h, w, 3) with channel stride 1 and pixel stride 3")
    n, h, w = (int(v) for v in rgb.shape[:3])
    fit = fit_args(h, w, H, W, box, rect, fill)
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=rgb.device)
    else:
        _cuda_u8(out, "out")
        if out.numel() != n * H * W * 3:
            raise ValueError("out must hold n * %d * %d * 3 bytes" % (H, W))
    with torch.cuda.device(rgb.device):
        if fit is None:
            check(lib().iiv_resize_frames(n, h, w, dptr(rgb), int(rgb.stride(0)), int(rgb.stride(1)), H, W, dptr(out),
                                          stream_ptr()))
        else:
            check(lib().iiv_resize_frames_fit(n, h, w, dptr(rgb), int(rgb.stride(0)), int(rgb.stride(1)), hptr(fit[0]), H, W,
                                              hptr(fit[1]), fit[2], dptr(out), stream_ptr()))
    return out


# ---- f11: YUV 4:2:0 sources ---------------------------------------------------------

# (y_off, ky, rv, gu, gv, bu) of include/iivision.h f11 by name; any other matrix is such a tuple
YUV_MATRICES = {
    "bt601": (16, 298, 409, -100, -208, 516),   # limited range; the default: the reference's material is SD
    "bt709": (16, 298, 459, -55, -136, 541),    # limited range
    "jpeg": (0, 256, 359, -88, -183, 454),      # full range, JFIF
}


def yuv_matrix(matrix):
    """A name of YUV_MATRICES or six integers -> the int32 array the C ABI takes (range errors are the library's)."""
    if isinstance(matrix, str):
        if matrix not in YUV_MATRICES:
            raise ValueError("unknown YUV matrix %r (one of %s, or six integers)" % (matrix, ", ".join(sorted(YUV_MATRICES))))
        matrix = YUV_MATRICES[matrix]
    m = np.asarray(matrix)
    if m.shape != (6,) or not np.issubdtype(m.dtype, np.integer):
        raise ValueError("a YUV matrix is six integers (y_off, ky, rv, gu, gv, bu)")
    return np.ascontiguousarray(m, dtype=np.int32)


def resize_frames_yuv420(y, u, v, size=RESIZE_SIZE, matrix="bt601", out=None, box=None, rect=None, fill=(0, 0, 0)):
    """resize_frames of the RGB frames that 4:2:0 planes define (include/iivision.h: iiv_resize_frames_yuv420), converted
    inside the resize's horizontal pass.  y: CUDA uint8 (n, h, w), unit pixel stride, any row and frame strides; u, v: CUDA
    uint8 (n, (h + 1) // 2, (w + 1) // 2) views with the same strides, pixel stride 1 (planar I420) or 2 (uv[..., 0] and
    uv[..., 1] of an (n, ch, cw, 2) NV12 tensor; swapped for NV21).  matrix: a name of YUV_MATRICES or (y_off, ky, rv, gu,
    gv, bu).  -> CUDA uint8 (n, H, W, 3); out, and the asynchrony on torch's current stream, exactly as resize_frames.
    box, rect, fill: as resize_frames', the box in pixels of the whole frame the planes define (odd offsets included)."""
    torch = _torch()
    H, W = (int(x) for x in size)
    m = yuv_matrix(matrix)
    for t, name in ((y, "y"), (u, "u"), (v, "v")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3):
            raise ValueError("%s must be a CUDA uint8 tensor of three dimensions" % name)
    n, h, w = (int(x) for x in y.shape)
    chroma = (n, (h + 1) // 2, (w + 1) // 2)
    if tuple(u.shape) != chroma or tuple(v.shape) != chroma:
        raise ValueError("u and v have shapes %s and %s; y %s needs chroma planes %s" % (tuple(u.shape), tuple(v.shape), (n, h, w), chroma))
    if _stride(y, 2, 1) != 1:
        raise ValueError("y must have pixel stride 1")
    ps = _stride(u, 2, _stride(v, 2, 1))
    c_rs = _stride(u, 1, _stride(v, 1, chroma[2] * ps))
    c_fs = _stride(u, 0, _stride(v, 0, chroma[1] * c_rs))
    if (_stride(v, 2, ps), _stride(v, 1, c_rs), _stride(v, 0, c_fs)) != (ps, c_rs, c_fs):
        raise ValueError("u and v must have the same strides")
    fit = fit_args(h, w, H, W, box, rect, fill)
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=y.device)
    else:
        _cuda_u8(out, "out")
        if out.numel() != n * H * W * 3:
            raise ValueError("out must hold n * %d * %d * 3 bytes" % (H, W))
    planes = (n, h, w, dptr(y), _stride(y, 0, h * _stride(y, 1, w)), _stride(y, 1, w), dptr(u), dptr(v), c_fs, c_rs, ps, hptr(m))
    with torch.cuda.device(y.device):
        if fit is None:
            check(lib().iiv_resize_frames_yuv420(*planes, H, W, dptr(out), stream_ptr()))
        else:
            check(lib().iiv_resize_frames_yuv420_fit(*planes, hptr(fit[0]), H, W, hptr(fit[1]), fit[2], dptr(out), stream_ptr()))
    return out
