// iiv_render.hip -- screen memory -> 560 x 192 RGB on gfx950 (f7: preview; include/iivision.h: iiv_render_rgb).
//
// The reference's colour model (colours.py:100-134: a sliding window of four dots, rotated by the dot's phase) prices every
// store of the encoder, but only per packed value (iiv_pixel_strings); this kernel applies it to whole screens, per screen
// row, as the header specifies it, so that what an opcode stream leaves on the screen can be looked at.
//
// Shape.  The kernel does nothing but stream: it writes 322 560 bytes per frame and reads 8 or 16 KiB.
//   * A wave takes a run of 64 consecutive units of sixteen dots = 48 output bytes each (iiv_render.h), whose output is ONE
//     contiguous, 16-byte-aligned run of 3 072 bytes -- also across frames, which follow each other without a gap.  A
//     lane's 48 bytes go through LDS (three 16-byte writes at 48 x lane) and leave as three 1 KiB store instructions, lane l
//     at base + 16 l: consecutive lanes, consecutive addresses, whole 128-byte lines.
//   * The run's at most three rows are staged in LDS and a unit's nineteen dots read from them as iiv_render.h says, which
//     iiv_render_error.hip shares; one palette lookup per dot.
//   * Waves are independent (private LDS, wave-level synchronisation only) and walk the run list with a grid stride.
// No scratch (tools/resource_usage.py), nothing allocated, nothing synchronised.
#include "iiv_render.h"

namespace iiv {

// main_mem / aux_mem: frame f's memory maps at + f * in_stride (8192 for a plain array of maps; the encoder's own copies lie
// one StreamState apart); rgb: [n_runs / 105][192][560][3]
template <int MODE>
__global__ __launch_bounds__(64 * kRenderWaves) void render_kernel(size_t n_runs, const uint8_t *__restrict__ main_mem,
                                                                   const uint8_t *__restrict__ aux_mem, size_t in_stride,
                                                                   const RenderPalette P, uint8_t *__restrict__ rgb)
{
    __shared__ __attribute__((aligned(16))) uint32_t out_s[kRenderWaves][64 * 12];
    __shared__ __attribute__((aligned(8))) uint8_t rows_s[kRenderWaves][3][kRenderSlot];
    __shared__ uint32_t pal_s[kRenderWaves][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t *out_w = out_s[wv];
    uint8_t(*rows_w)[kRenderSlot] = rows_s[wv];
    const uint32_t *pal_w = pal_s[wv];
    pal_s[wv][lane] = P.rgb[lane];
    render_zero_margins(rows_w, lane);
    const size_t n_waves = (size_t)gridDim.x * kRenderWaves;
    for (size_t run = (size_t)blockIdx.x * kRenderWaves + wv; run < n_runs; run += n_waves) {
        const size_t f = run / kRenderRunsPerFrame;
        const int u0 = 64 * (int)(run - f * kRenderRunsPerFrame);   // the run's first unit of the frame's 6 720
        const int y0 = u0 / 35;
        render_stage_rows<MODE>(rows_w, main_mem, aux_mem, f * in_stride, y0, lane);
        wave_lds_sync();
        {
            const int u = u0 + lane, y = u / 35, g = u - 35 * y;
            const uint32_t d = render_unit_dots(rows_w[y - y0], g);           // bit k: dot 16 g - 3 + k
            uint32_t o[12];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t c[4];
#pragma unroll
                for (int k = 0; k < 4; k++) c[k] = pal_w[16 * ((k + 1) & 3) + ((d >> (4 * q + k)) & 15u)];
                o[3 * q] = c[0] | (c[1] << 24);
                o[3 * q + 1] = (c[1] >> 8) | (c[2] << 16);
                o[3 * q + 2] = (c[2] >> 16) | (c[3] << 8);
            }
            uint4 *mine = reinterpret_cast<uint4 *>(out_w + 12 * lane);
            mine[0] = make_uint4(o[0], o[1], o[2], o[3]);
            mine[1] = make_uint4(o[4], o[5], o[6], o[7]);
            mine[2] = make_uint4(o[8], o[9], o[10], o[11]);
        }
        wave_lds_sync();
        uint4 *dst = reinterpret_cast<uint4 *>(rgb + run * (size_t)3072) + lane;
        const uint4 *src = reinterpret_cast<const uint4 *>(out_w) + lane;
#pragma unroll
        for (int k = 0; k < 3; k++) dst[64 * k] = src[64 * k];
        wave_lds_sync();   // (the next run's rows and bytes are written behind these reads)
    }
}

int render_rgb(int mode, const uint8_t palette_rgb[48], int n, const uint8_t *d_main, const uint8_t *d_aux, size_t in_stride,
               uint8_t *d_rgb, hipStream_t st)
{
    const RenderPalette P = make_render_palette(palette_rgb);
    const size_t n_runs = (size_t)n * kRenderRunsPerFrame;
    const dim3 grid(render_grid(n_runs));
    return launch(by_mode(mode, render_kernel<kDHGR>, render_kernel<kHGR>), "render_kernel launch", grid, dim3(64 * kRenderWaves), 0, st, n_runs,
                  d_main, d_aux, in_stride, P, d_rgb);
}

}  // namespace iiv

extern "C" int iiv_render_rgb(int mode, const uint8_t palette_rgb[48], int n, const uint8_t *d_main, const uint8_t *d_aux,
                              uint8_t *d_rgb, void *stream)
{
    if ((mode != IIV_HGR && mode != IIV_DHGR) || !palette_rgb || n < 0 || !d_main || !d_rgb || (mode == IIV_DHGR && !d_aux))
        return iiv::set_error(IIV_ERR_INVALID, "iiv_render_rgb: bad argument");
    if (((uintptr_t)d_main & 7) || (mode == IIV_DHGR && ((uintptr_t)d_aux & 7)) || ((uintptr_t)d_rgb & 15))
        return iiv::set_error(IIV_ERR_INVALID, "iiv_render_rgb: d_main / d_aux must be 8-byte aligned, d_rgb 16-byte aligned");
    if (n == 0) return IIV_OK;
    return iiv::render_rgb(mode, palette_rgb, n, d_main, d_aux, 8192, d_rgb, (hipStream_t)stream);
}
