// iiv_render_error.hip -- the rendered screen against a reference picture on gfx950 (f8: screen error; include/iivision.h:
// iiv_render_error).  Nine exact integer sums per frame: squared differences per dot, per quad of four dots and per unit of
// sixteen, for each of R, G, B.
//
// Shape.  render_kernel's (iiv_render.hip) with the direction of the big transfer reversed: it reads 322 560 (reference
// width 560) or 161 280 (width 280) bytes per frame and 8 or 16 KiB of screen memory, and writes 72.
//   * A wave takes a run of 64 consecutive units (iiv_render.h), stages the run's rows and reads each lane's nineteen dots
//     exactly as the render does.  The rendered RGB stays in registers: sixteen palette lookups per lane.
//   * The run's reference bytes are ONE contiguous, 16-byte-aligned block at d_ref + run * 3 072 (1 536 at width 280) -- also
//     across frames.  Lane l loads 16 bytes at base + 16 l (+ 1 024 k): whole 128-byte lines; they are issued before the
//     rows are staged, so both are in flight together.  The block goes through LDS to the 48 (24) bytes of the lane's
//     own unit: three 16-byte (8-byte) reads at 48 l (24 l).
//   * Per lane nine 32-bit sums (below 2^25), per wave nine DPP reductions (below 2^31), then ONE vector atomic instruction:
//     lanes 0 .. 8 add the wave's nine sums as 64-bit integers to the frame's 72 contiguous output bytes, which the call
//     zeroed on the stream in front of the kernel.  Integer sums: whatever order the 105 waves of a frame arrive in, the
//     result is the same.  945 such adds per frame against 330 KiB read.
//   * Waves are independent (private LDS, wave-level synchronisation only) and walk the run list with a grid stride.
// No workgroup barrier, no scratch (tools/resource_usage.py), nothing allocated, nothing synchronised.
#include "iiv_render.h"

namespace iiv {

// the sum over the wave, in an SGPR (sums below 2^31: no carry is lost)
__device__ static inline uint32_t wave_sum_u32(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);    // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false);   // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false);   // row_mirror: every lane holds its row's sum
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xf, 0xf, false);   // row_bcast:15 (row 0 adds 0)
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xf, 0xf, false);   // row_bcast:31: lane 63 holds the wave's
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// REFW: the reference's width, 560 (one pixel per dot) or 280 (one per two dots).  ref: [n_runs / 105][192][REFW][3];
// out: [n_runs / 105][3 levels][3 channels], zero when the kernel starts.  main_mem / aux_mem / in_stride: as render_kernel's.
template <int MODE, int REFW>
__global__ __launch_bounds__(64 * kRenderWaves) void render_error_kernel(size_t n_runs, const uint8_t *__restrict__ main_mem,
                                                                         const uint8_t *__restrict__ aux_mem, size_t in_stride,
                                                                         const RenderPalette P, const uint8_t *__restrict__ ref,
                                                                         unsigned long long *__restrict__ out)
{
    constexpr int kUnitBytes = REFW == 560 ? 48 : 24;        // a unit's reference bytes
    constexpr int kWords = kUnitBytes / 4;
    __shared__ __attribute__((aligned(16))) uint32_t ref_s[kRenderWaves][64 * kWords];
    __shared__ __attribute__((aligned(8))) uint8_t rows_s[kRenderWaves][3][kRenderSlot];
    __shared__ uint32_t pal_s[kRenderWaves][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t *ref_w = ref_s[wv];
    uint8_t(*rows_w)[kRenderSlot] = rows_s[wv];
    const uint32_t *pal_w = pal_s[wv];
    pal_s[wv][lane] = P.rgb[lane];
    render_zero_margins(rows_w, lane);
    const size_t n_waves = (size_t)gridDim.x * kRenderWaves;
    for (size_t run = (size_t)blockIdx.x * kRenderWaves + wv; run < n_runs; run += n_waves) {
        const size_t f = run / kRenderRunsPerFrame;
        const int u0 = 64 * (int)(run - f * kRenderRunsPerFrame);   // the run's first unit of the frame's 6 720
        const int y0 = u0 / 35;
        // the run's 64 x kUnitBytes reference bytes, 1 KiB per instruction (width 280: the second one is half a wave's)
        const uint4 *src = reinterpret_cast<const uint4 *>(ref + run * (size_t)(64 * kUnitBytes)) + lane;
        constexpr bool kWide = REFW == 560;
        const bool second = kWide || lane < 32;
        const uint4 in0 = src[0];
        uint4 in1 = make_uint4(0u, 0u, 0u, 0u), in2 = in1;
        if (second) in1 = src[64];
        if (kWide) in2 = src[128];
        render_stage_rows<MODE>(rows_w, main_mem, aux_mem, f * in_stride, y0, lane);
        uint4 *mid = reinterpret_cast<uint4 *>(ref_w) + lane;
        mid[0] = in0;
        if (second) mid[64] = in1;
        if (kWide) mid[128] = in2;
        wave_lds_sync();
        uint32_t s[9];
        {
            const int u = u0 + lane, y = u / 35, g = u - 35 * y;
            const uint32_t d = render_unit_dots(rows_w[y - y0], g);           // bit k: dot 16 g - 3 + k
            uint32_t r[kWords];
            if (REFW == 560) {
                const uint4 *mine = reinterpret_cast<const uint4 *>(ref_w + kWords * lane);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const uint4 v = mine[k];
                    r[4 * k] = v.x, r[4 * k + 1] = v.y, r[4 * k + 2] = v.z, r[4 * k + 3] = v.w;
                }
            } else {
                const uint2 *mine = reinterpret_cast<const uint2 *>(ref_w + kWords * lane);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const uint2 v = mine[k];
                    r[2 * k] = v.x, r[2 * k + 1] = v.y;
                }
            }
            uint32_t dot2[3] = {0u, 0u, 0u}, quad2[3] = {0u, 0u, 0u};
            int unit[3] = {0, 0, 0};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                int quad[3] = {0, 0, 0};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int i = 4 * q + k;                                  // the unit's dot; its phase (x + 1) & 3 = (k + 1) & 3
                    const uint32_t c = pal_w[16 * ((k + 1) & 3) + ((d >> i) & 15u)];
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        const int at = 3 * (REFW == 560 ? i : i / 2) + ch;    // R[x] = ref[x * REFW / 560]
                        const int diff = (int)((c >> (8 * ch)) & 0xffu) - (int)((r[at >> 2] >> (8 * (at & 3))) & 0xffu);
                        dot2[ch] += (uint32_t)(diff * diff);
                        quad[ch] += diff;
                    }
                }
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    quad2[ch] += (uint32_t)(quad[ch] * quad[ch]);
                    unit[ch] += quad[ch];
                }
            }
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                s[ch] = wave_sum_u32(dot2[ch]);
                s[3 + ch] = wave_sum_u32(quad2[ch]);
                s[6 + ch] = wave_sum_u32((uint32_t)(unit[ch] * unit[ch]));
            }
        }
        if (lane < 9) {
            uint32_t mine = s[0];
#pragma unroll
            for (int k = 1; k < 9; k++) mine = lane == k ? s[k] : mine;
            (void)__hip_atomic_fetch_add(out + f * 9 + lane, (unsigned long long)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        wave_lds_sync();   // (the next run's rows and reference bytes are written behind these reads)
    }
}

// frame f's memory maps at d_main / d_aux + f * in_stride bytes; arguments checked by the callers
int render_error(int mode, const uint8_t palette_rgb[48], int n, const uint8_t *d_main, const uint8_t *d_aux, size_t in_stride,
                 const uint8_t *d_ref, int ref_width, uint64_t *d_out, hipStream_t st)
{
    const RenderPalette P = make_render_palette(palette_rgb);
    const size_t n_runs = (size_t)n * kRenderRunsPerFrame;
    const dim3 grid(render_grid(n_runs)), block(64 * kRenderWaves);
    unsigned long long *out = reinterpret_cast<unsigned long long *>(d_out);
    IIV_HIP(hipMemsetAsync(d_out, 0, (size_t)n * 72, st));
    const bool wide = ref_width == 560;
    const auto kernel = by_mode(mode, wide ? render_error_kernel<kDHGR, 560> : render_error_kernel<kDHGR, 280>,
                                wide ? render_error_kernel<kHGR, 560> : render_error_kernel<kHGR, 280>);
    return launch(kernel, "render_error_kernel launch", grid, block, 0, st, n_runs, d_main, d_aux, in_stride, P, d_ref, out);
}

}  // namespace iiv

extern "C" int iiv_render_error(int mode, const uint8_t palette_rgb[48], int n, const uint8_t *d_main, const uint8_t *d_aux,
                                const uint8_t *d_ref, int ref_width, uint64_t *d_out, void *stream)
{
    if ((mode != IIV_HGR && mode != IIV_DHGR) || !palette_rgb || n < 0 || !d_main || !d_ref || !d_out || (mode == IIV_DHGR && !d_aux))
        return iiv::set_error(IIV_ERR_INVALID, "iiv_render_error: bad argument");
    if (ref_width != 280 && ref_width != 560) return iiv::set_error(IIV_ERR_INVALID, "iiv_render_error: ref_width must be 280 or 560");
    if (((uintptr_t)d_main & 7) || (mode == IIV_DHGR && ((uintptr_t)d_aux & 7)) || ((uintptr_t)d_ref & 15) || ((uintptr_t)d_out & 7))
        return iiv::set_error(IIV_ERR_INVALID,
                              "iiv_render_error: d_main / d_aux / d_out must be 8-byte aligned, d_ref 16-byte aligned");
    if (n == 0) return IIV_OK;
    return iiv::render_error(mode, palette_rgb, n, d_main, d_aux, 8192, d_ref, ref_width, d_out, (hipStream_t)stream);
}
