// iiv_temporal.hip -- the temporal hold (f14; include/iivision.h: iiv_temporal_hold): per pixel, along the frames of a clip, the
// held value stays where the source is within `lo` of it, follows the source where it is more than `hi` away, and moves part of
// the way in between.  The reference has nothing on the time axis: its frames reach bmp2dhr as the decoder delivers them.
//
// Shape.  A work item is (clip, run of lanes) -- lanes of 12 bytes, runs and the capped grid are iiv_clip.h's.  The kernel only
// streams: every byte is read once and written once; frames are sequential per pixel and independent across pixels and clips.
//   * The held values of a lane's four pixels live in three registers over the whole frame loop; the state is read in front of
//     the loop (not with `first`) and written behind it.
//   * The only loop-carried dependence is the held value.  The source of frame t + kTemporalRing is loaded when frame t is
//     taken out of a register ring of kTemporalRing frames (3 dwords each), so the chain per frame is VALU work and one LDS
//     lookup, not a memory latency.  In place (d_out == d_src) a lane stores frame t behind its own load of frame t and of
//     every frame the ring holds; no lane touches another lane's bytes.
//   * w(d) is a table of 256 u16 built on the host from (lo, hi), passed by value and staged in LDS once per workgroup: no
//     division on the device.  A channel is y = (h (256 - w) + x w + 128) >> 8, which is h + (((x - h) w + 128) >> 8) with the
//     floor towards minus infinity (h 256 is a multiple of 256) and never negative: at most 255 * 256 + 128 < 2^16.  The first
//     frame of a `first` call takes w = 256 for every pixel: y = x whatever the registers held.
//   * Counts: a pixel is held where w == 0 and passed where w == 256; a wave counts each class of each of its four pixel slots
//     with a ballot and lane 0 adds the three sums to the frame's entry: one atomic add per class per wave and frame.  Integer
//     adds in any order give the same counts.  The entries are cleared on the caller's stream in front of the launch.
// Nothing is allocated, nothing synchronised, nothing kept between calls.
#include "iiv_clip.h"
#include "iiv_host.h"

namespace iiv {

namespace {

constexpr int kTemporalRing = 8;            // frames whose source is in flight ahead of the one being computed

struct TemporalWeights {
    uint16_t w[256];   // w(d) of f14: 0 for d <= lo, 256 for d > hi, 1..255 between
};

template <bool kCount>
__global__ __launch_bounds__(kClipThreads) void temporal_kernel(size_t n_items, size_t runs, size_t lanes, int n_frames, const uint8_t *src,
                                                                size_t src_clip_stride, size_t src_frame_stride, uint8_t *out,
                                                                size_t out_clip_stride, size_t out_frame_stride, uint8_t *state,
                                                                size_t state_stride, int first, const TemporalWeights W, uint32_t *counts)
{
    __shared__ uint16_t w_s[256];
    const int tid = threadIdx.x;
    w_s[tid] = W.w[tid];   // (kClipThreads == 256)
    __syncthreads();
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t clip = item / runs;
        const size_t lane = (item - clip * runs) * kClipThreads + tid;
        const bool active = lane < lanes;
        const size_t at = active ? lane * (kClipLanePixels * 3) : 0;   // (an idle lane computes on zeros and stores nothing)
        const uint8_t *s = src + clip * src_clip_stride + at;
        uint8_t *o = out + clip * out_clip_stride + at;
        uint8_t *st = state + clip * state_stride + at;
        Dwords3 h = {{0, 0, 0}};
        if (active && !first) h = *reinterpret_cast<const Dwords3 *>(st);
        Dwords3 ring[kTemporalRing];
#pragma unroll
        for (int k = 0; k < kTemporalRing; k++) {
            ring[k] = Dwords3{{0, 0, 0}};
            if (active && k < n_frames) ring[k] = *reinterpret_cast<const Dwords3 *>(s + (size_t)k * src_frame_stride);
        }
        for (int t0 = 0; t0 < n_frames; t0 += kTemporalRing) {
#pragma unroll
            for (int k = 0; k < kTemporalRing; k++) {
                const int t = t0 + k;
                if (t >= n_frames) break;   // (the same in every thread)
                const Dwords3 x = ring[k];
                if (active && t + kTemporalRing < n_frames)
                    ring[k] = *reinterpret_cast<const Dwords3 *>(s + (size_t)(t + kTemporalRing) * src_frame_stride);
                const bool pass_all = first && t == 0;
                uint32_t y[kClipLanePixels * 3];
                uint32_t n_held = 0, n_passed = 0;
#pragma unroll
                for (int p = 0; p < kClipLanePixels; p++) {
                    uint32_t xc[3], hc[3], d = 0;
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        xc[c] = clip_byte(x, 3 * p + c);
                        hc[c] = clip_byte(h, 3 * p + c);
                        const uint32_t a = xc[c] > hc[c] ? xc[c] - hc[c] : hc[c] - xc[c];
                        d = a > d ? a : d;
                    }
                    const uint32_t w = pass_all ? 256u : w_s[d];
#pragma unroll
                    for (int c = 0; c < 3; c++) y[3 * p + c] = (hc[c] * (256u - w) + xc[c] * w + 128u) >> 8;
                    if (kCount) {
                        n_held += __popcll(__ballot(active && w == 0));
                        n_passed += __popcll(__ballot(active && w == 256u));
                    }
                }
#pragma unroll
                for (int i = 0; i < 3; i++) h.v[i] = clip_pack4(y[4 * i], y[4 * i + 1], y[4 * i + 2], y[4 * i + 3]);
                if (active) *reinterpret_cast<Dwords3 *>(o + (size_t)t * out_frame_stride) = h;
                if (kCount) {
                    const uint32_t n_all = kClipLanePixels * (uint32_t)__popcll(__ballot(active));
                    if ((tid & 63) == 0 && active) {   // (lanes are taken in order: a wave with an active lane has lane 0 active)
                        uint32_t *c = counts + (clip * (size_t)n_frames + (size_t)t) * 3;
                        atomicAdd(c + 0, n_held);
                        atomicAdd(c + 1, n_all - n_held - n_passed);
                        atomicAdd(c + 2, n_passed);
                    }
                }
            }
        }
        if (active) *reinterpret_cast<Dwords3 *>(st) = h;
    }
}

}  // namespace

}  // namespace iiv

using namespace iiv;

extern "C" {

int iiv_temporal_hold(int n_clips, int n_frames, long pixels, const uint8_t *d_src, size_t src_clip_stride, size_t src_frame_stride,
                      uint8_t *d_out, size_t out_clip_stride, size_t out_frame_stride, uint8_t *d_state, size_t state_stride,
                      int first, int lo, int hi, uint32_t *d_counts, void *stream)
{
    if (int rc = clip_refuse("iiv_temporal_hold", n_clips, n_frames, pixels, 40,
                             (uintptr_t)d_src | (uintptr_t)d_out | (uintptr_t)d_state | (uintptr_t)d_counts | src_clip_stride |
                                 src_frame_stride | out_clip_stride | out_frame_stride | state_stride,
                             {src_frame_stride, out_frame_stride}))
        return rc;
    if (lo < 0 || hi > 255 || lo > hi) return set_error(IIV_ERR_INVALID, "iiv_temporal_hold: 0 <= lo <= hi <= 255, got (%d, %d)", lo, hi);
    if (n_clips > 1 && state_stride < (size_t)pixels * 3)
        return set_error(IIV_ERR_INVALID, "iiv_temporal_hold: state_stride is below the %zu bytes of a held frame", (size_t)pixels * 3);
    if (n_clips == 0 || n_frames == 0) return IIV_OK;
    if (!d_src || !d_out || !d_state) return set_error(IIV_ERR_INVALID, "iiv_temporal_hold: a NULL pointer");
    TemporalWeights W;
    for (int d = 0; d < 256; d++) W.w[d] = (uint16_t)(d <= lo ? 0 : d > hi ? 256 : 256 * (d - lo) / (hi - lo + 1));
    const size_t lanes = clip_lanes(pixels), runs = clip_runs(lanes);
    const size_t n_items = (size_t)n_clips * runs;
    hipStream_t st = (hipStream_t)stream;
    if (d_counts) IIV_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_clips * (size_t)n_frames * 3 * sizeof(uint32_t), st));
    return launch(d_counts ? temporal_kernel<true> : temporal_kernel<false>, "temporal_kernel launch", dim3(clip_grid(n_items)),
                  dim3(kClipThreads), 0, st, n_items, runs, lanes, n_frames, d_src, src_clip_stride, src_frame_stride, d_out,
                  out_clip_stride, out_frame_stride, d_state, state_stride, first ? 1 : 0, W, d_counts);
}

}  // extern "C"
