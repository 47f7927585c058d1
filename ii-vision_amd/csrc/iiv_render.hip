// iiv_render.hip -- screen memory -> 560 x 192 RGB on gfx950 (f7: preview; include/iivision.h: iiv_render_rgb).
//
// The reference's colour model (colours.py:100-134: a sliding window of four dots, rotated by the dot's phase) prices every
// store of the encoder, but only per packed value (iiv_pixel_strings); this kernel applies it to whole screens, per screen
// row, as the header specifies it, so that what an opcode stream leaves on the screen can be looked at.
//
// Shape.  The kernel does nothing but stream: it writes 322 560 bytes per frame and reads 8 or 16 KiB.
//   * A frame is 6 720 UNITS of sixteen dots = 48 output bytes (35 per row), and 6 720 = 105 x 64: a wave takes 64
//     consecutive units, whose output is ONE contiguous, 16-byte-aligned run of 3 072 bytes -- also across frames, which
//     follow each other without a gap.  A lane's 48 bytes go through LDS (three 16-byte writes at 48 x lane) and leave as
//     three 1 KiB store instructions, lane l at base + 16 l: consecutive lanes, consecutive addresses, whole 128-byte lines.
//   * 64 units touch at most three rows.  Thirty lanes load them once, one or two aligned dwords each (the screen holes are
//     never read), and leave every row in LDS as 80 bytes of seven dots -- what a DHGR row is once aux and main bytes are
//     interleaved; an HGR row is brought into the same form there (data bits doubled, shifted by the palette bit, bit 6 of
//     the byte to the left in the uncovered dot) -- between eight zero bytes on either side: the dots left of the row,
//     and what an aligned read runs into behind it.  A unit then reads two aligned dwords, squeezes four bytes into 28 dots
//     and shifts its nineteen (three to the left of its first) down.
//   * The palette is in LDS as 64 words, [phase (x + 1) & 3][window] -> R | G << 8 | B << 16 of rol4(window, phase), built on
//     the host per call and passed by value: one lookup per dot, its phase static (a unit starts at a multiple of four).
//   * Waves are independent (private LDS, wave-level synchronisation only) and walk the run list with a grid stride.
// No scratch (tools/resource_usage.py), nothing allocated, nothing synchronised.
#include "iiv_host.h"
#include "iiv_stream.h"

namespace iiv {

constexpr int kRenderWaves = 4;               // waves per workgroup
constexpr int kRenderRunsPerFrame = 105;      // 64-unit runs per frame: 192 rows x 35 units / 64
constexpr int kRenderSlot = 96;               // LDS bytes per staged row: 8 zero, 80 of seven dots, 8 zero

struct RenderPalette {
    uint32_t rgb[64];     // [(x + 1) & 3][window of dots x - 3 .. x] -> R | G << 8 | B << 16 of the dot's colour value
};

static RenderPalette make_render_palette(const uint8_t pal[48])
{
    RenderPalette p;
    for (int ph = 0; ph < 4; ph++)
        for (int w = 0; w < 16; w++) {
            const int v = ((w << ph) | (w >> (4 - ph))) & 15;   // rol4(w, ph) (colours.py:87-97)
            p.rgb[16 * ph + w] = (uint32_t)pal[3 * v] | ((uint32_t)pal[3 * v + 1] << 8) | ((uint32_t)pal[3 * v + 2] << 16);
        }
    return p;
}

__device__ static inline int render_row_offset(int y)  // y_to_base_addr(y, 0) - 0x2000 (screen.py:16-22)
{
    return 1024 * (y & 7) + 128 * ((y & 63) >> 3) + 40 * (y >> 6);
}

// HGR: a byte's fourteen dots (screen.py:743-789 per byte) as two bytes of seven: bit k -> dots 2k, 2k + 1; with the palette
// bit set everything moves one dot right, `left6` (bit 6 of the byte to the left) shows in dot 0 and the fifteenth dot is dropped
__device__ static inline uint32_t hgr_byte_dots(uint32_t b, uint32_t left6)
{
    uint32_t x = b & 0x7fu;
    x = (x | (x << 4)) & 0x0f0fu;
    x = (x | (x << 2)) & 0x3333u;
    x = (x | (x << 1)) & 0x5555u;
    x *= 3u;
    if (b & 0x80u) x = ((x << 1) | left6) & 0x3fffu;
    return (x & 0x7fu) | ((x >> 7) << 8);
}

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
    if (lane < 6) *reinterpret_cast<uint2 *>(&rows_w[lane % 3][lane < 3 ? 0 : 88]) = make_uint2(0u, 0u);
    const size_t n_waves = (size_t)gridDim.x * kRenderWaves;
    for (size_t run = (size_t)blockIdx.x * kRenderWaves + wv; run < n_runs; run += n_waves) {
        const size_t f = run / kRenderRunsPerFrame;
        const int u0 = 64 * (int)(run - f * kRenderRunsPerFrame);   // the run's first unit of the frame's 6 720
        const int y0 = u0 / 35;
        if (lane < 30) {
            // row y0 + lane / 10 (the last run of a frame touches two: row 191 is then staged twice), bytes 4 j .. 4 j + 3 of its 40
            const int r = lane / 10, j = lane - 10 * r;
            const int y = min(y0 + r, 191);
            const size_t at = f * in_stride + (size_t)(render_row_offset(y) + 4 * j);
            const uint32_t m = *reinterpret_cast<const uint32_t *>(main_mem + at);
            uint32_t lo, hi;
            if (MODE == kDHGR) {
                const uint32_t a = *reinterpret_cast<const uint32_t *>(aux_mem + at) & 0x7f7f7f7fu, mm = m & 0x7f7f7f7fu;
                lo = (a & 0xffu) | ((mm & 0xffu) << 8) | ((a & 0xff00u) << 8) | ((mm & 0xff00u) << 16);
                hi = ((a >> 16) & 0xffu) | ((mm >> 8) & 0xff00u) | ((a >> 8) & 0xff0000u) | (mm & 0xff000000u);
            } else {
                const uint32_t left = j ? *reinterpret_cast<const uint32_t *>(main_mem + at - 4) : 0u;   // (never in front of the row)
                lo = hgr_byte_dots(m & 0xffu, (left >> 30) & 1u) | (hgr_byte_dots((m >> 8) & 0xffu, (m >> 6) & 1u) << 16);
                hi = hgr_byte_dots((m >> 16) & 0xffu, (m >> 14) & 1u) | (hgr_byte_dots(m >> 24, (m >> 22) & 1u) << 16);
            }
            *reinterpret_cast<uint2 *>(&rows_w[r][8 + 8 * j]) = make_uint2(lo, hi);
        }
        wave_lds_sync();
        {
            const int u = u0 + lane, y = u / 35, g = u - 35 * y;
            // byte b of the staged row holds dots 7 b .. 7 b + 6; the unit shows dots 16 g .. 16 g + 15 and looks at three more
            // to their left: four bytes from bf = floor((16 g - 3) / 7) (-1 for g = 0: the zero byte in front of the row)
            const int bf = (16 * g + 4) / 7 - 1;
            const uint8_t *p = &rows_w[y - y0][8 + bf];
            const uint32_t mis = (uint32_t)(8 + bf) & 3u;
            const uint32_t *two = reinterpret_cast<const uint32_t *>(p - mis);   // (4-aligned only: two dword reads)
            const uint32_t v = __builtin_amdgcn_alignbyte(two[1], two[0], mis);
            const uint32_t d28 = (v & 0x7fu) | ((v >> 1) & 0x3f80u) | ((v >> 2) & 0x1fc000u) | ((v >> 3) & 0xfe00000u);
            const uint32_t d = d28 >> (uint32_t)(16 * g - 3 - 7 * bf);        // bit k: dot 16 g - 3 + k
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
    // enough workgroups to fill the chip eight waves per SIMD deep; larger batches walk the runs with a grid stride
    const size_t blocks = (n_runs + kRenderWaves - 1) / kRenderWaves;
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048));
    if (mode == kDHGR)
        hipLaunchKernelGGL(render_kernel<kDHGR>, grid, dim3(64 * kRenderWaves), 0, st, n_runs, d_main, d_aux, in_stride, P, d_rgb);
    else
        hipLaunchKernelGGL(render_kernel<kHGR>, grid, dim3(64 * kRenderWaves), 0, st, n_runs, d_main, d_aux, in_stride, P, d_rgb);
    return hip_check(hipGetLastError(), "render_kernel launch");
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
