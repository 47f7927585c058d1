// iiv_frontend.h -- what the four converters from RGB frames to screen memory share (iiv_ingest.hip, iiv_diffuse.hip,
// iiv_mono.hip, iiv_direct.hip): the screen's row arithmetic, the ordered-dither offsets and the palette's linear forms on
// the host; on the device the arg-min over those forms, the 42-byte source group and the screen-hole kernel's launch.
// Everything on the device is inlined into the kernels that use it, and their code is instruction for instruction what it
// was when each file held its own copy: profiles/frontend_isa_identity.txt.  (What did NOT stay identical when shared, and so
// is still spelt twice: the staged source stream of the two colour error-diffusion kernels -- the same record.)
// The first part is plain host arithmetic (no HIP type), so that a host compiler can build it alone
// (tests/test_frontend_host.py prints it); the device part is seen by hipcc only.
#pragma once
#include <stdint.h>

namespace iiv {

#ifdef __HIPCC__
__host__ __device__
#endif
static inline int y_to_offset(int y)  // y_to_base_addr(y, 0) - 0x2000 (screen.py:16-22)
{
    return 1024 * (y % 8) + 128 * ((y % 64) / 8) + 40 * (y / 64);
}

// the ordered-dither offset of (y & 3) * 4 + (x & 3): floor((2 Bayer - 15) * amplitude / 16), floor towards minus infinity
static inline void dither_offsets(int amplitude, int32_t out[16])
{
    static const int bayer[16] = {0, 8, 2, 10, 12, 4, 14, 6, 3, 11, 1, 9, 15, 7, 13, 5};
    for (int c = 0; c < 16; c++) out[c] = ((2 * bayer[c] - 15) * amplitude + 16 * 256) / 16 - 256;
}

// The palette as the colour kernels use it (built on the host per call, passed by value): the nearest colour is an arg-min of
// linear forms, key_c = 16 (K_c - 4 R_c r - 8 G_c g - 6 B_c b) + c (iiv_ingest.hip, top of the file)
struct PaletteForms {
    int32_t k[16];        // 16 (2 R^2 + 4 G^2 + 3 B^2) + colour value
    int32_t a[16], b[16], c[16];   // -16 * 4 R, -16 * 8 G, -16 * 6 B
    uint32_t bc[16];      // the last two as a pair of 16-bit halves (both fit: 128 x 255, 96 x 255 < 2^15): v_dot2c_i32_i16's operand
    uint32_t rgb[16];     // R | G << 8 | B << 16
};

static inline PaletteForms make_palette_forms(const uint8_t pal[48])
{
    PaletteForms p;
    for (int c = 0; c < 16; c++) {
        const int R = pal[3 * c], G = pal[3 * c + 1], B = pal[3 * c + 2];
        p.k[c] = 16 * (2 * R * R + 4 * G * G + 3 * B * B) + c;
        p.a[c] = -64 * R;
        p.b[c] = -128 * G;
        p.c[c] = -96 * B;
        p.bc[c] = (uint32_t)(uint16_t)(int16_t)(-128 * G) | ((uint32_t)(uint16_t)(int16_t)(-96 * B) << 16);
        p.rgb[c] = (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16);
    }
    return p;
}

}  // namespace iiv

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace iiv {

// Zeroes the screen holes of n_frames memory maps (offsets 120..127, 248..255 of every page; d_aux's too in DHGR) on `st`:
// the one screen-hole kernel, its grid and its launch (iiv_ingest.hip)
int zero_screen_holes(int mode, int n_frames, uint8_t *d_main, uint8_t *d_aux, hipStream_t st);

// The sixteen K_c in vector registers: a VOP3 instruction reads ONE scalar register, so mad(r, A_c, K_c) with both constants
// in SGPRs costs a v_mov besides -- with K_c in a VGPR a colour is exactly three v_mad_i32_i24 (the compiler otherwise
// builds it from two multiplies, a multiply-add and a three-operand add plus the moves: 4.5 instructions and 2.6 moves)
struct Kv {
    int k[16];
};
__device__ static inline Kv kv_of(const PaletteForms &P)
{
    Kv v;
#pragma unroll
    for (int c = 0; c < 16; c++) {
        v.k[c] = P.k[c];
        asm volatile("" : "+v"(v.k[c]));
    }
    return v;
}

// key of colour c for the pixel (r, g, b) = 16 * (distance - the term common to all colours) + c
//     = (K_c + r * (-64 R_c)) + (g, b) . (-128 G_c, -96 B_c):
// a v_mad_i32_i24 into a fresh register and a v_dot2c_i32_i16 that accumulates in place (16-bit pairs, exact 32-bit sum; g, b
// are clamped to 0..255, the coefficients fit 16 bits) -- two instructions instead of three multiply-adds.  (Both products
// in dot form, (r, g) . (..) + (b, 0) . (..), compile to the accumulate-in-place form too and then need a copy of K_c each:
// three again.)  DHGR: the nearest of the sixteen colours (ties to the lower colour value).
typedef short v2s __attribute__((ext_vector_type(2)));
__device__ static inline int dist_key(const PaletteForms &P, int kc, int c, int r, v2s gb)
{
    return __builtin_amdgcn_sdot2(gb, __builtin_bit_cast(v2s, P.bc[c]), __mul24(r, P.a[c]) + kc, false);
}
__device__ static inline int nearest16(const PaletteForms &P, const Kv &kv, int r, int g, int b)
{
    const v2s gb = __builtin_bit_cast(v2s, (uint32_t)g | ((uint32_t)b << 16));
    int m = 0x7fffffff;
#pragma unroll
    for (int c = 0; c < 16; c++) m = min(m, dist_key(P, kv.k[c], c, r, gb));
    return m & 15;
}
// The same with three v_mad_i32_i24 per colour, for the error-diffusion kernels: a lane's pixels there are one dependent chain,
// and the wait states between a v_dot2c and the minimum that reads it cost that kernel more (1.6 %, same-box A/B) than the
// sixteen instructions save.  Three rounds of sixteen independent multiply-adds with ONE compiler barrier between rounds (the
// barrier keeps the compiler from re-associating a colour's chain into mad + 2 mul + add3; one asm statement per round rather
// than per colour, because the hazard recogniser puts an s_nop behind every inline-asm statement)
__device__ static inline int nearest16_mad(const PaletteForms &P, const Kv &kv, int r, int g, int b)
{
    int t[16];
#pragma unroll
    for (int c = 0; c < 16; c++) t[c] = __mul24(r, P.a[c]) + kv.k[c];
    asm("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]), "+v"(t[8]), "+v"(t[9]),
             "+v"(t[10]), "+v"(t[11]), "+v"(t[12]), "+v"(t[13]), "+v"(t[14]), "+v"(t[15]));
#pragma unroll
    for (int c = 0; c < 16; c++) t[c] = __mul24(g, P.b[c]) + t[c];
    asm("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]), "+v"(t[8]), "+v"(t[9]),
             "+v"(t[10]), "+v"(t[11]), "+v"(t[12]), "+v"(t[13]), "+v"(t[14]), "+v"(t[15]));
    int m = 0x7fffffff;
#pragma unroll
    for (int c = 0; c < 16; c++) m = min(m, __mul24(b, P.c[c]) + t[c]);
    return m & 15;
}

// HGR: for both palette bits, (distance term << 2 | pattern) of the nearest of the four colours the bit allows
// (black 0, violet 3 | blue 6, green 12 | orange 9, white 15; ties to the lower pattern)
__device__ static inline void nearest4x2(const PaletteForms &P, const Kv &kv, int r, int g, int b, int &key0, int &key1)
{
    // the six colours HGR can show
    constexpr int col[6] = {0, 3, 12, 15, 6, 9};
    const v2s gb = __builtin_bit_cast(v2s, (uint32_t)g | ((uint32_t)b << 16));
    int t[6];
#pragma unroll
    for (int j = 0; j < 6; j++) t[j] = dist_key(P, kv.k[col[j]], col[j], r, gb) >> 4;   // (>> 4: the colour value leaves, the distance term stays exact)
    const int f0 = t[0], f3 = t[1], f12 = t[2], f15 = t[3], f6 = t[4], f9 = t[5];
    const int b0 = f0 * 4, w3 = f15 * 4 + 3;
    key0 = min(min(b0, f3 * 4 + 1), min(f12 * 4 + 2, w3));
    key1 = min(min(b0, f6 * 4 + 1), min(f9 * 4 + 2, w3));
}

// N dwords of source bytes, funnel-shifted so that byte 0 is the first byte of a thread's group.  (byte_at is a member on
// purpose: as a free function over the array the compiler commutes the adds that consume it.)
template <int N> struct SourceBytes {
    uint32_t q[N];
    __device__ int byte_at(int nb) const { return (int)((q[nb >> 2] >> (8 * (nb & 3))) & 255u); }
};
// The 42 source bytes at frame + off (off even; seven colour pixels, or fourteen mono dots): aligned dwords from off & ~3,
// then a funnel shift by 0 or 16 bits.  (Eleven dwords from the aligned base never leave the frame: a group at an odd halfword
// ends with its eleventh dword or has 42 bytes behind it.)
__device__ static inline void load_group42(const uint8_t *frame, int off, uint32_t (&q)[11])
{
    const uint8_t *src = frame + (size_t)off;
    const uint32_t *w32 = reinterpret_cast<const uint32_t *>(src - (off & 2));
    uint32_t w[11];
#pragma unroll
    for (int i = 0; i < 11; i++) w[i] = w32[i];
    const uint32_t sh = ((uint32_t)off & 2u) * 8u;
#pragma unroll
    for (int i = 0; i < 10; i++) q[i] = __builtin_amdgcn_alignbit(w[i + 1], w[i], sh);
    q[10] = w[10] >> sh;
}

// mean of the two source pixels of group pixel GP, three channels in one v_lerp_u8: bytes 6 GP .. 6 GP + 5 of cur
template <int GP> __device__ static inline uint32_t mean_of(const uint32_t (&cur)[11])
{
    constexpr int oa = 6 * GP, ob = 6 * GP + 3;
    const uint32_t A = (oa & 3) ? __builtin_amdgcn_alignbit(cur[(oa >> 2) + 1], cur[oa >> 2], (oa & 3) * 8) : cur[oa >> 2];
    const uint32_t B = (ob & 3) ? __builtin_amdgcn_alignbit(cur[(ob >> 2) + 1 > 10 ? 10 : (ob >> 2) + 1], cur[ob >> 2], (ob & 3) * 8) : cur[ob >> 2];
    return __builtin_amdgcn_lerp(A, B, 0x01010101u);
}

}  // namespace iiv
#endif  // __HIPCC__
