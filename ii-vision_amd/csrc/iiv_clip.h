// iiv_clip.h -- what the stages that run along the frames of a clip share (iiv_temporal.hip, iiv_levels.hip).  A clip is
// n_clips x n_frames dense RGB frames of `pixels` pixels; clip and frame strides are free multiples of 4 bytes.  A lane owns four
// pixels: three dwords, 12 contiguous bytes per frame (a wave 768, a workgroup 3 KiB); a run is a workgroup's lanes of one frame;
// a stage's work items (clip x run, clip x frame, ...: its own) are walked with a grid stride under kClipGridCap workgroups.
// The first part is plain C++ (no HIP type): a host compiler builds it alone (tests/test_clip_host.py).  The device part is
// inlined into its kernels and left their code instruction for instruction what it was: profiles/clip_isa_identity.txt.
#pragma once
#include <initializer_list>
#include <stdint.h>
#include "../../include/iivision.h"

namespace iiv {

int set_error(int code, const char *fmt, ...);   // (iiv_api.hip's; a program that builds this header alone supplies its own)

constexpr int kClipThreads = 256;           // lanes of a workgroup
constexpr int kClipLanePixels = 4;          // pixels of a lane: 12 bytes = three dwords per frame
constexpr int kClipGridCap = 2048;          // workgroups of a launch; the items beyond are reached by the grid stride

// What every clip entry point `name` refuses before it looks at anything of its own, in this order; IIV_OK when the call may go
// on.  pixels is at most 2^max_pixels_log2; `aligned` is the OR of every pointer and every stride of the call; each of
// frame_strides must hold a frame.  (Empty work -- IIV_OK -- and NULL pointers come behind the stage's own refusals, there.)
static inline int clip_refuse(const char *name, int n_clips, int n_frames, long pixels, int max_pixels_log2, uintptr_t aligned,
                              std::initializer_list<size_t> frame_strides)
{
    if (n_clips < 0 || n_frames < 0) return set_error(IIV_ERR_INVALID, "%s: n_clips or n_frames < 0", name);
    if (pixels <= 0 || pixels % kClipLanePixels)
        return set_error(IIV_ERR_INVALID, "%s: pixels must be a positive multiple of 4, got %ld", name, pixels);
    if (pixels > (long)1 << max_pixels_log2) return set_error(IIV_ERR_INVALID, "%s: pixels above 2^%d", name, max_pixels_log2);
    if (aligned & 3) return set_error(IIV_ERR_INVALID, "%s: every pointer and every stride must be 4-byte aligned", name);
    for (size_t stride : frame_strides)
        if (stride < (size_t)pixels * 3)
            return set_error(IIV_ERR_INVALID, "%s: a frame stride is below the %zu bytes of a frame", name, (size_t)pixels * 3);
    return IIV_OK;
}

// lanes of a frame, runs of lanes, and the workgroups that walk n_items
static inline size_t clip_lanes(long pixels) { return (size_t)pixels / kClipLanePixels; }
static inline size_t clip_runs(size_t lanes) { return (lanes + kClipThreads - 1) / kClipThreads; }
static inline unsigned clip_grid(size_t n_items) { return (unsigned)(n_items < (size_t)kClipGridCap ? n_items : (size_t)kClipGridCap); }

}  // namespace iiv

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace iiv {

// a lane's 12 bytes of one frame, and byte i (0..11) of them: channel i % 3 of pixel i / 3
struct alignas(4) Dwords3 { uint32_t v[3]; };
__device__ static inline uint32_t clip_byte(const Dwords3 &a, int i) { return (a.v[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// four byte values back into dword i of them: v[i] = clip_pack4(y[4 i], y[4 i + 1], y[4 i + 2], y[4 i + 3]).  (A dword at a time
// and by value on purpose: one function over the array of twelve moves instructions in temporal_kernel<true>, the same record.)
__device__ static inline uint32_t clip_pack4(uint32_t y0, uint32_t y1, uint32_t y2, uint32_t y3) { return y0 | y1 << 8 | y2 << 16 | y3 << 24; }

}  // namespace iiv
#endif  // __HIPCC__
