// iiv_levels.hip -- picture levels (f15; include/iivision.h: iiv_levels_histogram, iiv_levels_auto, iiv_levels_apply): the
// histograms of every frame, black and white points from a histogram, and a per-channel table with a 3 x 3 matrix behind it.  The
// reference hands this stage to bmp2dhr; what it does itself of the kind is the audio track's normalisation (audio.py:60-78).
//
// Histogram (a frame's lanes of 12 bytes, runs of lanes and the capped grid, here and below: iiv_clip.h).  A work item is one
// (clip, frame) and belongs to one workgroup, so nothing is shared between workgroups:
//   * the 4 x 256 bins live in LDS (4 KiB) and are zero whenever a workgroup starts an item: it clears them once in front of the
//     loop and again while it stores them; a trip over the frame takes one run of lanes;
//   * the bins leave by plain stores, 1 KiB per channel: no global atomics, no memset, every entry written;
//   * a count is an LDS atomic add.  The Makefile turns the compiler's own atomic optimiser off, so where every lane holds the
//     same value (a flat frame, a letterbox bar) 64 adds to one address would run one after the other.  levels_count therefore
//     peels ONE value off per count: the lanes that hold lane 0's value are counted with a ballot and added by lane 0 alone, the
//     others add for themselves.  A flat wave costs one add, a noisy one what it cost before plus a compare and a ballot
//     (IIV_LEVELS_NO_COMBINE builds the kernel without: tools/levels_probe.py measures both).  Integer adds in any
//     order give the same counts: the result does not depend on the peel, only the time does.
//   A frame far above 560x192 still is one workgroup's: its time grows with its pixels while other CUs may idle (DESIGN.md 31
//   says what that costs).
//
// Apply.  The kernel only streams: every byte is read once and written once.
//   * One 12-byte load and one 12-byte store per lane and frame; in place (d_out == d_src) a lane stores behind its own load
//     and touches no other lane's bytes.  The next frame's load is issued in front of the current frame's store.
//   * The clip's 768 table bytes and 9 weights are staged in LDS when a workgroup meets a clip it has not staged (with both
//     strides 0: once).
//   * A work item is (clip, run of lanes, range of kLevelsApplyFrames frames): a single clip of many frames fills the device as
//     a batch of many clips does.
// Nothing is allocated, nothing synchronised, nothing kept between calls.
#include "iiv_clip.h"
#include "iiv_host.h"

namespace iiv {

namespace {

constexpr int kLevelsApplyFrames = 8;       // frames of one apply item

// one count of value v into bins[0..255] by every `active` lane (called by the whole wave; lanes are taken in order, so a wave
// with an active lane has lane 0 active)
__device__ inline void levels_count(uint32_t *bins, uint32_t v, bool active, bool lane0)
{
#ifdef IIV_LEVELS_NO_COMBINE
    if (active) atomicAdd(bins + v, 1u);
#else
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    const bool same = active && v == first;
    const uint32_t n_same = (uint32_t)__popcll(__ballot(same));
    if (lane0 ? active : (active && !same)) atomicAdd(bins + v, lane0 ? n_same : 1u);
#endif
}

__global__ __launch_bounds__(kClipThreads) void levels_histogram_kernel(size_t n_items, int n_frames, size_t lanes, const uint8_t *src,
                                                                        size_t src_clip_stride, size_t src_frame_stride, uint32_t *hist)
{
    __shared__ uint32_t bins[4 * 256];
    const int tid = threadIdx.x;
    const bool lane0 = (tid & 63) == 0;
#pragma unroll
    for (int c = 0; c < 4; c++) bins[c * 256 + tid] = 0;   // (kClipThreads == 256)
    __syncthreads();
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t clip = item / (size_t)n_frames;
        const size_t frame = item - clip * (size_t)n_frames;
        const uint8_t *s = src + clip * src_clip_stride + frame * src_frame_stride;
        Dwords3 next = {{0, 0, 0}};   // (an idle lane computes on zeros and counts nothing)
        if ((size_t)tid < lanes) next = *reinterpret_cast<const Dwords3 *>(s + (size_t)tid * (kClipLanePixels * 3));
        for (size_t base = 0; base < lanes; base += kClipThreads) {   // (the same trips in every thread)
            const size_t lane = base + tid;
            const bool active = lane < lanes;
            const Dwords3 x = next;    // the next trip's load is in flight under this trip's counts
            if (lane + kClipThreads < lanes)
                next = *reinterpret_cast<const Dwords3 *>(s + (lane + kClipThreads) * (kClipLanePixels * 3));
#pragma unroll
            for (int p = 0; p < kClipLanePixels; p++) {
                const uint32_t r = clip_byte(x, 3 * p), g = clip_byte(x, 3 * p + 1), b = clip_byte(x, 3 * p + 2);
                const uint32_t y = (77u * r + 150u * g + 29u * b + 128u) >> 8;
                levels_count(bins, r, active, lane0);
                levels_count(bins + 256, g, active, lane0);
                levels_count(bins + 512, b, active, lane0);
                levels_count(bins + 768, y, active, lane0);
            }
        }
        __syncthreads();
        uint32_t *o = hist + item * (4 * 256);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            o[c * 256 + tid] = bins[c * 256 + tid];
            bins[c * 256 + tid] = 0;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kClipThreads) void levels_apply_kernel(size_t n_items, size_t runs, size_t ranges, size_t lanes, int n_frames,
                                                                    const uint8_t *src, size_t src_clip_stride, size_t src_frame_stride,
                                                                    uint8_t *out, size_t out_clip_stride, size_t out_frame_stride,
                                                                    const uint8_t *lut, size_t lut_stride, const uint8_t *matrix,
                                                                    size_t matrix_stride)
{
    __shared__ uint32_t lut_s[3 * 256 / 4];
    __shared__ int m_s[9];
    const uint8_t *lut_b = reinterpret_cast<const uint8_t *>(lut_s);
    const int tid = threadIdx.x;
    const bool per_clip = lut_stride != 0 || matrix_stride != 0;
    size_t staged = ~(size_t)0;
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {   // (the same trips in every thread)
        const size_t clip = item / (runs * ranges);
        const size_t rest = item - clip * (runs * ranges);
        const size_t run = rest / ranges;
        const int t0 = (int)(rest - run * ranges) * kLevelsApplyFrames;
        const int t1 = t0 + kLevelsApplyFrames < n_frames ? t0 + kLevelsApplyFrames : n_frames;
        const size_t tables = per_clip ? clip : 0;
        if (tables != staged) {   // (uniform in the workgroup)
            __syncthreads();      // (nobody still reads the tables of the item before)
            if (tid < 192) lut_s[tid] = reinterpret_cast<const uint32_t *>(lut + clip * lut_stride)[tid];
            else if (tid < 192 + 9) m_s[tid - 192] = reinterpret_cast<const int16_t *>(matrix + clip * matrix_stride)[tid - 192];
            __syncthreads();
            staged = tables;
        }
        const size_t lane = run * kClipThreads + tid;
        if (lane >= lanes) continue;   // (no barrier below in this trip)
        const size_t at = lane * (kClipLanePixels * 3);
        const uint8_t *s = src + clip * src_clip_stride + at;
        uint8_t *o = out + clip * out_clip_stride + at;
        int m[9];
#pragma unroll
        for (int i = 0; i < 9; i++) m[i] = m_s[i];
        Dwords3 next = *reinterpret_cast<const Dwords3 *>(s + (size_t)t0 * src_frame_stride);
        for (int t = t0; t < t1; t++) {
            const Dwords3 x = next;
            if (t + 1 < t1) next = *reinterpret_cast<const Dwords3 *>(s + (size_t)(t + 1) * src_frame_stride);
            uint32_t y[kClipLanePixels * 3];
#pragma unroll
            for (int p = 0; p < kClipLanePixels; p++) {
                int a[3];
#pragma unroll
                for (int c = 0; c < 3; c++) a[c] = lut_b[c * 256 + clip_byte(x, 3 * p + c)];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    // clamp((v >> 8), 0, 255) as clamp(v, 0, 65535) >> 8: the same value, and not the shift-then-saturate shape that
                    // hipcc turns into v_ashr_pk_u8_i32, whose result it ORs with the other two bytes as if the instruction
                    // cleared the upper half of its destination -- on the device it does not (bytes 2 and 3 of a dword came
                    // out with stale bits)
                    const int v = m[3 * c] * a[0] + m[3 * c + 1] * a[1] + m[3 * c + 2] * a[2] + 128;
                    y[3 * p + c] = (uint32_t)(v < 0 ? 0 : v > 65535 ? 65535 : v) >> 8;
                }
            }
            Dwords3 r;
#pragma unroll
            for (int i = 0; i < 3; i++) r.v[i] = clip_pack4(y[4 * i], y[4 * i + 1], y[4 * i + 2], y[4 * i + 3]);
            *reinterpret_cast<Dwords3 *>(o + (size_t)t * out_frame_stride) = r;
        }
    }
}

}  // namespace

}  // namespace iiv

using namespace iiv;

extern "C" {

int iiv_levels_histogram(int n_clips, int n_frames, long pixels, const uint8_t *d_src, size_t src_clip_stride,
                         size_t src_frame_stride, uint32_t *d_hist, void *stream)
{
    if (int rc = clip_refuse("iiv_levels_histogram", n_clips, n_frames, pixels, 31,   // (2^31: a count fits its uint32)
                             (uintptr_t)d_src | (uintptr_t)d_hist | src_clip_stride | src_frame_stride, {src_frame_stride}))
        return rc;
    if (n_clips == 0 || n_frames == 0) return IIV_OK;
    if (!d_src || !d_hist) return set_error(IIV_ERR_INVALID, "iiv_levels_histogram: a NULL pointer");
    const size_t n_items = (size_t)n_clips * (size_t)n_frames;
    return launch(levels_histogram_kernel, "levels_histogram_kernel launch", dim3(clip_grid(n_items)), dim3(kClipThreads), 0,
                  (hipStream_t)stream, n_items, n_frames, clip_lanes(pixels), d_src, src_clip_stride, src_frame_stride, d_hist);
}

int iiv_levels_auto(const uint64_t hist[256], uint32_t lo_ppm, uint32_t hi_ppm, int *black, int *white)
{
    if (!hist || !black || !white) return set_error(IIV_ERR_INVALID, "iiv_levels_auto: a NULL pointer");
    if (lo_ppm > 500000 || hi_ppm > 500000)
        return set_error(IIV_ERR_INVALID, "iiv_levels_auto: lo_ppm and hi_ppm are at most 500000, got (%u, %u)", lo_ppm, hi_ppm);
    const uint64_t limit = (uint64_t)1 << 43;
    uint64_t total = 0;
    for (int v = 0; v < 256; v++) {
        if (hist[v] > limit) return set_error(IIV_ERR_INVALID, "iiv_levels_auto: a total above 2^43");
        total += hist[v];   // (at most 256 * 2^43)
    }
    if (total > limit) return set_error(IIV_ERR_INVALID, "iiv_levels_auto: a total above 2^43");
    const uint64_t k_lo = total * lo_ppm / 1000000, k_hi = total * hi_ppm / 1000000;
    int b = 0, w = 255;
    if (total) {
        uint64_t cum = 0;   // cum(v)
        for (b = 0; b < 256; b++) {
            cum += hist[b];
            if (cum > k_lo) break;
        }
        uint64_t tail = 0;  // total - cum(v - 1)
        for (w = 255; w >= 0; w--) {
            tail += hist[w];
            if (tail > k_hi) break;
        }
        if (w <= b) b = 0, w = 255;
    }
    *black = b;
    *white = w;
    return IIV_OK;
}

int iiv_levels_apply(int n_clips, int n_frames, long pixels, const uint8_t *d_src, size_t src_clip_stride, size_t src_frame_stride,
                     uint8_t *d_out, size_t out_clip_stride, size_t out_frame_stride, const uint8_t *d_lut, size_t lut_stride,
                     const int16_t *d_matrix, size_t matrix_stride, void *stream)
{
    if (int rc = clip_refuse("iiv_levels_apply", n_clips, n_frames, pixels, 40,
                             (uintptr_t)d_src | (uintptr_t)d_out | (uintptr_t)d_lut | (uintptr_t)d_matrix | src_clip_stride |
                                 src_frame_stride | out_clip_stride | out_frame_stride | lut_stride | matrix_stride,
                             {src_frame_stride, out_frame_stride}))
        return rc;
    if ((lut_stride != 0 && lut_stride < 768) || (matrix_stride != 0 && matrix_stride < 20))
        return set_error(IIV_ERR_INVALID, "iiv_levels_apply: lut_stride is 0 or at least 768, matrix_stride 0 or at least 20, got (%zu, %zu)",
                         lut_stride, matrix_stride);
    if (n_clips == 0 || n_frames == 0) return IIV_OK;
    if (!d_src || !d_out || !d_lut || !d_matrix) return set_error(IIV_ERR_INVALID, "iiv_levels_apply: a NULL pointer");
    const size_t lanes = clip_lanes(pixels), runs = clip_runs(lanes);
    const size_t ranges = ((size_t)n_frames + kLevelsApplyFrames - 1) / kLevelsApplyFrames;
    const size_t n_items = (size_t)n_clips * runs * ranges;
    return launch(levels_apply_kernel, "levels_apply_kernel launch", dim3(clip_grid(n_items)), dim3(kClipThreads), 0,
                  (hipStream_t)stream, n_items, runs, ranges, lanes, n_frames, d_src, src_clip_stride, src_frame_stride, d_out,
                  out_clip_stride, out_frame_stride, d_lut, lut_stride, reinterpret_cast<const uint8_t *>(d_matrix), matrix_stride);
}

}  // extern "C"
