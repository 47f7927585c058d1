// iiv_direct.hip -- RGB frames -> memory maps chosen THROUGH the colour model on gfx950 (f10: direct ingest;
// include/iivision.h: iiv_frames_to_memory_maps_direct).  For every screen row the byte row whose rendered
// dots (f7's sliding window) are nearest the dithered source, found exactly: a forward pass over the row's 560 dots with
// the last three dots as the state, then a backtrace that fixes the bytes in descending significance and takes 0 whenever a
// least-cost completion exists.  tests/direct_model.py states the same trellis in numpy and is held to the contract's
// global rule by exhaustive search.
//
// Shape.  One screen row per LANE; rows are independent, so nothing is exchanged and nothing synchronised.
//   * The path sums are registers: 8 in DHGR; in HGR 8 per palette bit of the byte, and over the first four dots of a byte
//     -- the dots whose windows look at the byte to the left -- 8 more per palette bit p' of THAT byte: p' is more
//     significant than its data bits, so its two branches stay apart until the window has left that byte and meet behind
//     the fourth dot, ties to p' = 0.  An HGR dot is a new data bit or a copy of the dot before it (palette bit 0: the odd
//     dots of a byte's fourteen, 1: the even ones, dot 0 copying the last dot of the byte to the left); a state that breaks
//     a copy is unreachable (kDirectInf) and costs no instruction: which ones are is known at compile time.
//   * A dot's cost against colour value v is (|P_v|^2 - 2 P_v . T) + |T|^2; the last term is common to every candidate, so
//     the sums carry the first and the row adds the second at the end: sixteen values of three multiply-adds per dot, each
//     window's value a static register (the dot loop is unrolled over the four phases).
//   * Back-pointers stay on chip: one bit per dot and state in LDS, a dword column per lane ([word][lane]: no bank is
//     shared).  DHGR: 140 words per row, 64 rows per workgroup (35 KiB).  HGR: ten words per byte -- four dots of 32
//     states, ten of 16, the 16 meeting bits -- 400 per row, 32 rows per workgroup (50 KiB).
//   * The row's cost goes to the frame's 64-bit sum by one vector atomic add per row (integers: any order gives the same
//     sum); the call zeroes the sums on the stream in front of the kernel.  The screen holes are written by the frame's
//     first 64 rows.
// No allocation, no scratch (profiles/direct_resource_usage.txt), no barrier.
#include "iiv_frontend.h"
#include "iiv_render.h"
#include <utility>

namespace iiv {

constexpr int kDirectInf = 1 << 30;   // above every path sum (|sum| < 560 * 3 * 2 * 255^2 < 2^28), with room for a few costs on top

struct DirectPalette {
    int32_t k[16];                    // R^2 + G^2 + B^2 of colour value v
    int32_t r[16], g[16], b[16];      // -2 R, -2 G, -2 B
    int32_t dither[16];               // ordered-dither offset of (y & 3) * 4 + (quad & 3): floor((2 Bayer - 15) * amplitude / 16)
};

static DirectPalette make_direct_palette(const uint8_t pal[48], int dither)
{
    DirectPalette p;
    dither_offsets(dither, p.dither);
    for (int v = 0; v < 16; v++) {
        const int R = pal[3 * v], G = pal[3 * v + 1], B = pal[3 * v + 2];
        p.k[v] = R * R + G * G + B * B;
        p.r[v] = -2 * R, p.g[v] = -2 * G, p.b[v] = -2 * B;
    }
    return p;
}

__device__ constexpr int direct_rol4(int w, int n) { return ((w << n) | (w >> (4 - n))) & 15; }

// the four dots of quad q of a row: T = clamp(source + d, 0, 255) per channel, the source pixel x * REFW / 560 of dot x
template <int REFW>
__device__ static inline void direct_targets(const uint8_t *__restrict__ row, int q, int d, int (&t)[4][3])
{
    if (REFW == 560) {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(row) + 3 * q;     // twelve bytes at 12 q
        const uint32_t w[3] = {p[0], p[1], p[2]};
#pragma unroll
        for (int j = 0; j < 12; j++) t[j / 3][j % 3] = min(max((int)((w[j >> 2] >> (8 * (j & 3))) & 255u) + d, 0), 255);
    } else {
        const uint16_t *p = reinterpret_cast<const uint16_t *>(row) + 3 * q;     // six bytes at 6 q: two pixels, two dots each
        const uint32_t h[3] = {p[0], p[1], p[2]};
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const int v = min(max((int)((h[j >> 1] >> (8 * (j & 1))) & 255u) + d, 0), 255);
            t[2 * (j / 3)][j % 3] = t[2 * (j / 3) + 1][j % 3] = v;
        }
    }
}

// cv[v] = |P_v|^2 - 2 P_v . T; returns |T|^2
__device__ static inline uint32_t direct_costs(const DirectPalette &P, const int (&t)[3], int (&cv)[16])
{
#pragma unroll
    for (int v = 0; v < 16; v++) cv[v] = __mul24(t[2], P.b[v]) + (__mul24(t[1], P.g[v]) + (__mul24(t[0], P.r[v]) + P.k[v]));
    return (uint32_t)(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
}

constexpr int kDirectRowsDHGR = 64, kDirectRowsHGR = 32;   // rows (lanes) per workgroup

// One dot.  F[s]: the least sum over the rows that end in the dots s = a | b << 1 | c << 2 (c the newest).  The new state s
// has the window w = dropped dot | s << 1 and came from w & 7; bit s of the result: the dropped dot is 1 (ties to 0).
// PH = (x + 1) & 3; COPY: the new dot repeats the one before it.
template <int PH, bool COPY>
__device__ static inline uint32_t direct_step(int (&F)[8], const int (&cv)[16])
{
    int Fn[8];
    uint32_t bits = 0;
#pragma unroll
    for (int s = 0; s < 8; s++) {
        if (COPY && ((s >> 1) & 1) != ((s >> 2) & 1)) {
            Fn[s] = kDirectInf;
            continue;
        }
        const int w0 = 2 * s, w1 = 2 * s + 1;
        const int v0 = F[w0 & 7] + cv[direct_rol4(w0, PH)], v1 = F[w1 & 7] + cv[direct_rol4(w1, PH)];
        const bool one = v1 < v0;
        Fn[s] = one ? v1 : v0;
        bits |= (uint32_t)one << s;
    }
#pragma unroll
    for (int s = 0; s < 8; s++) F[s] = Fn[s];
    return bits;
}

// the dither offsets of row y's four quad columns
__device__ static inline void direct_dither_row(const DirectPalette &P, int y, int (&d)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int a = (y & 1) ? P.dither[4 + j] : P.dither[j], b = (y & 1) ? P.dither[12 + j] : P.dither[8 + j];
        d[j] = (y & 2) ? b : a;
    }
}
// (a row's quads take d[0], d[1], d[2], d[3], d[0], ...: the loops below keep the next quad's in d[0] by rotating the four registers --
// indexed by the quad number the compiler puts them into scratch)
__device__ static inline void direct_dither_rotate(int (&d)[4], int by)
{
    for (int k = 0; k < by; k++) {
        const int d0 = d[0];
        d[0] = d[1], d[1] = d[2], d[2] = d[3], d[3] = d0;
    }
}

// rows 0 .. 63 of a frame zero its 64 eight-byte screen holes, in every bank
__device__ static inline void direct_holes(uint8_t *main_frame, uint8_t *aux_frame, int y)
{
    if (y < 64) {
        const int at = (y >> 1) * 256 + ((y & 1) ? 248 : 120);
        *reinterpret_cast<uint2 *>(main_frame + at) = make_uint2(0u, 0u);
        if (aux_frame) *reinterpret_cast<uint2 *>(aux_frame + at) = make_uint2(0u, 0u);
    }
}


// rgb: [n_rows / 192][192][REFW][3]; cost: [n_rows / 192], zero when the kernel starts, or NULL
template <int REFW>
__global__ __launch_bounds__(kDirectRowsDHGR) void direct_dhgr_kernel(size_t n_rows, const uint8_t *__restrict__ rgb, const DirectPalette P,
                                                                      uint8_t *__restrict__ main_mem, uint8_t *__restrict__ aux_mem,
                                                                      unsigned long long *__restrict__ cost)
{
    __shared__ uint32_t back_s[140][kDirectRowsDHGR];     // [quad][lane]: byte k = the dropped dots of dot 4 quad + k, bit s = state s
    const int lane = threadIdx.x;
    const size_t id = (size_t)blockIdx.x * kDirectRowsDHGR + lane;
    if (id >= n_rows) return;
    const size_t f = id / 192;
    const int y = (int)(id - f * 192);
    const uint8_t *row = rgb + id * (size_t)(REFW * 3);
    int dy[4];
    direct_dither_row(P, y, dy);
    int F[8];
#pragma unroll
    for (int s = 0; s < 8; s++) F[s] = s ? kDirectInf : 0;            // left of the row: dots of 0
    uint32_t common = 0;
    for (int q = 0; q < 140; q++) {
        int t[4][3], cv[16];
        direct_targets<REFW>(row, q, dy[0], t);
        direct_dither_rotate(dy, 1);
        uint32_t bp;
        common += direct_costs(P, t[0], cv);
        bp = direct_step<1, false>(F, cv);
        common += direct_costs(P, t[1], cv);
        bp |= direct_step<2, false>(F, cv) << 8;
        common += direct_costs(P, t[2], cv);
        bp |= direct_step<3, false>(F, cv) << 16;
        common += direct_costs(P, t[3], cv);
        bp |= direct_step<0, false>(F, cv) << 24;
        back_s[q][lane] = bp;
    }
    int s = 0, best = F[0];
#pragma unroll
    for (int k = 1; k < 8; k++)
        if (F[k] < best) best = F[k], s = k;                          // ties to the smaller state: its newest dot is the most significant
    if (cost) (void)__hip_atomic_fetch_add(cost + f, (unsigned long long)(uint32_t)(best + (int)common), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint8_t *main_frame = main_mem + f * 8192, *aux_frame = aux_mem + f * 8192;
    const int at = render_row_offset(y);
    for (int i = 79; i >= 0; i--) {                                   // the row's byte sequence aux[0], main[0], aux[1], ...
        uint32_t b = 0;
#pragma unroll
        for (int j = 6; j >= 0; j--) {
            const int x = 7 * i + j;
            b |= (uint32_t)(s >> 2) << j;
            const uint32_t bits = back_s[x >> 2][lane] >> (8 * (x & 3));
            s = ((s << 1) | (int)((bits >> s) & 1u)) & 7;
        }
        ((i & 1) ? main_frame : aux_frame)[at + (i >> 1)] = (uint8_t)b;
    }
    direct_holes(main_frame, aux_frame, y);
}

// dot DD of the 28 of bytes 2 i2, 2 i2 + 1 of an HGR row (28 i2 is a multiple of four: the phase (x + 1) & 3 is (DD + 1) & 3).
// back: the lane's column of back-pointer words, at the pair's first; its words are kDirectRowsHGR apart.
template <int REFW, int DD>
__device__ __forceinline__ void direct_hgr_dot(const DirectPalette &P, const uint8_t *__restrict__ row, const int (&dy)[4], int i2, int (&F)[4][8],
                                               int (&t)[4][3], uint32_t &held, uint32_t &common, uint32_t *back)
{
    constexpr int PH = (DD + 1) & 3, r = DD % 14, word = 10 * (DD / 14);
    constexpr bool copy0 = (r & 1) == 1, copy1 = (r & 1) == 0;       // the dot repeats the one before it under palette bit 0 / 1
    if (DD % 4 == 0) {
        const int q = 7 * i2 + DD / 4;
        direct_targets<REFW>(row, q, dy[(DD / 4) & 3], t);                 // (dy[0]: the pair's first quad)
    }
    int cv[16];
    common += direct_costs(P, t[DD & 3], cv);
    if (r < 4) {
        const uint32_t bits = direct_step<PH, copy0>(F[0], cv) | (direct_step<PH, copy0>(F[1], cv) << 8) |
                              (direct_step<PH, copy1>(F[2], cv) << 16) | (direct_step<PH, copy1>(F[3], cv) << 24);
        back[(word + r) * kDirectRowsHGR] = bits;
    } else {
        const uint32_t bits = direct_step<PH, copy0>(F[0], cv) | (direct_step<PH, copy1>(F[2], cv) << 8);
        if (r & 1) back[(word + 4 + ((r - 4) >> 1)) * kDirectRowsHGR] = held | (bits << 16);
        else held = bits;
    }
    if (r == 3) {                                                     // the branches of p' meet, ties to p' = 0
        uint32_t mb = 0;
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int s = 0; s < 8; s++) {
                const bool one = F[2 * p + 1][s] < F[2 * p][s];
                F[2 * p][s] = one ? F[2 * p + 1][s] : F[2 * p][s];
                mb |= (uint32_t)one << (8 * p + s);
            }
        back[(word + 9) * kDirectRowsHGR] = mb;
    }
    if (r == 13) {                                                    // the byte's end: its palette bit becomes the next byte's p'
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const int g0 = F[0][s], g1 = F[2][s];
            F[0][s] = g0, F[1][s] = g1, F[2][s] = g0, F[3][s] = g1;
        }
    }
}
template <int REFW, int... DD>
__device__ __forceinline__ void direct_hgr_dots(std::integer_sequence<int, DD...>, const DirectPalette &P, const uint8_t *__restrict__ row,
                                                const int (&dy)[4], int i2, int (&F)[4][8], int (&t)[4][3], uint32_t &held, uint32_t &common,
                                                uint32_t *back)
{
    (direct_hgr_dot<REFW, DD>(P, row, dy, i2, F, t, held, common, back), ...);
}

// HGR.  F[2 p + p'][s]: p the palette bit of the byte the dot is in, p' that of the byte to its left (only over a byte's
// first four dots; behind them p' = 0 holds the sum of the better branch).
template <int REFW>
__global__ __launch_bounds__(kDirectRowsHGR) void direct_hgr_kernel(size_t n_rows, const uint8_t *__restrict__ rgb, const DirectPalette P,
                                                                    uint8_t *__restrict__ main_mem, unsigned long long *__restrict__ cost)
{
    // per byte ten words: 0..3 dots 0..3 (bit 8 (2 p + p') + s), 4..8 dots 4..13 in pairs (bit 16 (dot & 1) + 8 p + s), 9 the
    // meeting of p' (bit 8 p + s: the better branch is p' = 1)
    __shared__ uint32_t back_s[400][kDirectRowsHGR];
    const int lane = threadIdx.x;
    const size_t id = (size_t)blockIdx.x * kDirectRowsHGR + lane;
    if (id >= n_rows) return;
    const size_t f = id / 192;
    const int y = (int)(id - f * 192);
    const uint8_t *row = rgb + id * (size_t)(REFW * 3);
    int dy[4];
    direct_dither_row(P, y, dy);
    int F[4][8];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int s = 0; s < 8; s++) F[q][s] = ((q & 1) || s) ? kDirectInf : 0;   // left of the row: dots of 0 and no byte (p' = 0)
    uint32_t common = 0;
    for (int i2 = 0; i2 < 20; i2++) {                                 // two bytes: 28 dots, seven quads, every phase static
        int t[4][3];
        uint32_t held = 0;
        direct_hgr_dots<REFW>(std::make_integer_sequence<int, 28>{}, P, row, dy, i2, F, t, held, common, &back_s[20 * i2][lane]);
        direct_dither_rotate(dy, 3);                                  // seven quads on
    }
    // the last byte's palette bit (F[0]: 0, F[1]: 1), the smaller first; then the smaller state
    int p = 0, s = 0, best = F[0][0];
#pragma unroll
    for (int k = 1; k < 16; k++)
        if (F[k >> 3][k & 7] < best) best = F[k >> 3][k & 7], p = k >> 3, s = k & 7;
    if (cost) (void)__hip_atomic_fetch_add(cost + f, (unsigned long long)(uint32_t)(best + (int)common), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint8_t *main_frame = main_mem + f * 8192;
    const int at = render_row_offset(y);
    for (int i = 39; i >= 0; i--) {
        int left = 0;
        uint32_t dots = 0;
        for (int r = 13; r >= 0; r--) {
            if (r == 3) left = (int)((back_s[10 * i + 9][lane] >> (8 * p + s)) & 1u);
            dots |= (uint32_t)(s >> 2) << r;
            const uint32_t bits = r < 4 ? back_s[10 * i + r][lane] >> (8 * (2 * p + left))
                                        : back_s[10 * i + 4 + ((r - 4) >> 1)][lane] >> (16 * (r & 1) + 8 * p);
            s = ((s << 1) | (int)((bits >> s) & 1u)) & 7;
        }
        // data bit k is dot 2 k (palette bit 0) or 2 k + 1 (1; bit 6: dot 13, its second dot belongs to the next byte or is dropped)
        uint32_t e = p ? dots >> 1 : dots, b = (uint32_t)p << 7;
#pragma unroll
        for (int k = 0; k < 7; k++) b |= ((e >> (2 * k)) & 1u) << k;
        main_frame[at + i] = (uint8_t)b;
        p = left;
    }
    direct_holes(main_frame, nullptr, y);
}

// arguments checked by the caller
int frames_to_memory_maps_direct(int mode, const uint8_t palette_rgb[48], int n, const uint8_t *d_rgb, int ref_width, int dither,
                                 uint8_t *d_main, uint8_t *d_aux, uint64_t *d_cost, hipStream_t st)
{
    const DirectPalette P = make_direct_palette(palette_rgb, dither);
    const size_t n_rows = (size_t)n * 192;
    unsigned long long *cost = reinterpret_cast<unsigned long long *>(d_cost);
    if (d_cost) IIV_HIP(hipMemsetAsync(d_cost, 0, (size_t)n * sizeof(uint64_t), st));
    const bool wide = ref_width == 560;
    if (mode == kDHGR)
        return launch(wide ? direct_dhgr_kernel<560> : direct_dhgr_kernel<280>, "direct_dhgr_kernel launch",
                      dim3((unsigned)((n_rows + kDirectRowsDHGR - 1) / kDirectRowsDHGR)), dim3(kDirectRowsDHGR), 0, st, n_rows, d_rgb, P, d_main,
                      d_aux, cost);
    return launch(wide ? direct_hgr_kernel<560> : direct_hgr_kernel<280>, "direct_hgr_kernel launch",
                  dim3((unsigned)((n_rows + kDirectRowsHGR - 1) / kDirectRowsHGR)), dim3(kDirectRowsHGR), 0, st, n_rows, d_rgb, P, d_main, cost);
}

}  // namespace iiv

extern "C" int iiv_frames_to_memory_maps_direct(int mode, const uint8_t palette_rgb[48], int n_frames, const uint8_t *d_rgb,
                                                int ref_width, int dither, uint8_t *d_main, uint8_t *d_aux, uint64_t *d_cost,
                                                void *stream)
{
    if ((mode != IIV_HGR && mode != IIV_DHGR) || !palette_rgb || n_frames < 0 || !d_rgb || !d_main || (mode == IIV_DHGR && !d_aux))
        return iiv::set_error(IIV_ERR_INVALID, "iiv_frames_to_memory_maps_direct: bad argument");
    if (ref_width != 280 && ref_width != 560)
        return iiv::set_error(IIV_ERR_INVALID, "iiv_frames_to_memory_maps_direct: ref_width must be 280 or 560");
    if (dither < 0 || dither > 255)
        return iiv::set_error(IIV_ERR_INVALID, "iiv_frames_to_memory_maps_direct: dither must be 0..255 (no error diffusion)");
    if (((uintptr_t)d_rgb & 3) || ((uintptr_t)d_main & 7) || (mode == IIV_DHGR && ((uintptr_t)d_aux & 7)) || ((uintptr_t)d_cost & 7))
        return iiv::set_error(IIV_ERR_INVALID,
                              "iiv_frames_to_memory_maps_direct: d_rgb must be 4-byte aligned, d_main / d_aux / d_cost 8-byte aligned");
    if (n_frames == 0) return IIV_OK;
    return iiv::frames_to_memory_maps_direct(mode, palette_rgb, n_frames, d_rgb, ref_width, dither, d_main, d_aux, d_cost,
                                             (hipStream_t)stream);
}
