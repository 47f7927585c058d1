// iiv_render.h -- what the kernels that look at whole screens share (f7: iiv_render.hip writes the screen's RGB, f8:
// iiv_render_error.hip measures it against a reference picture): the run geometry, the palette as the kernels take it, the
// staging of a run's screen rows in LDS and a unit's nineteen dots.  One copy, so that both see the same screen.
//
//   * A frame is 6 720 UNITS of sixteen dots (35 per row), and 6 720 = 105 x 64: a wave takes a RUN of 64 consecutive units.
//   * 64 units touch at most three rows.  Thirty lanes load them once, one or two aligned dwords each (the screen holes are
//     never read), and leave every row in LDS as 80 bytes of seven dots -- what a DHGR row is once aux and main bytes are
//     interleaved; an HGR row is brought into the same form there (data bits doubled, shifted by the palette bit, bit 6 of
//     the byte to the left in the uncovered dot) -- between eight zero bytes on either side: the dots left of the row,
//     and what an aligned read runs into behind it.  A unit then reads two aligned dwords, squeezes four bytes into 28 dots
//     and shifts its nineteen (three to the left of its first) down.
//   * The palette is 64 words, [phase (x + 1) & 3][window] -> R | G << 8 | B << 16 of rol4(window, phase), built on the host
//     per call and passed by value: one lookup per dot, its phase static (a unit starts at a multiple of four).
#pragma once

#include "iiv_host.h"
#include "iiv_stream.h"

namespace iiv {

constexpr int kRenderWaves = 4;               // waves per workgroup
constexpr int kRenderRunsPerFrame = 105;      // 64-unit runs per frame: 192 rows x 35 units / 64
constexpr int kRenderSlot = 96;               // LDS bytes per staged row: 8 zero, 80 of seven dots, 8 zero

struct RenderPalette {
    uint32_t rgb[64];     // [(x + 1) & 3][window of dots x - 3 .. x] -> R | G << 8 | B << 16 of the dot's colour value
};

static inline RenderPalette make_render_palette(const uint8_t pal[48])
{
    RenderPalette p;
    for (int ph = 0; ph < 4; ph++)
        for (int w = 0; w < 16; w++) {
            const int v = ((w << ph) | (w >> (4 - ph))) & 15;   // rol4(w, ph) (colours.py:87-97)
            p.rgb[16 * ph + w] = (uint32_t)pal[3 * v] | ((uint32_t)pal[3 * v + 1] << 8) | ((uint32_t)pal[3 * v + 2] << 16);
        }
    return p;
}

// enough workgroups to fill the chip eight waves per SIMD deep; larger batches walk the runs with a grid stride
static inline unsigned render_grid(size_t n_runs)
{
    const size_t blocks = (n_runs + kRenderWaves - 1) / kRenderWaves;
    return (unsigned)(blocks < 2048 ? blocks : 2048);
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

// once per wave, before its first run: the eight zero bytes on either side of the three staged rows
__device__ static inline void render_zero_margins(uint8_t (*rows_w)[kRenderSlot], int lane)
{
    if (lane < 6) *reinterpret_cast<uint2 *>(&rows_w[lane % 3][lane < 3 ? 0 : 88]) = make_uint2(0u, 0u);
}

// the rows y0 .. y0 + 2 of the frame whose memory maps start at main_mem / aux_mem + frame_at, into rows_w (lanes 0 .. 29; the
// caller synchronises the wave's LDS behind it)
template <int MODE>
__device__ static inline void render_stage_rows(uint8_t (*rows_w)[kRenderSlot], const uint8_t *__restrict__ main_mem,
                                                const uint8_t *__restrict__ aux_mem, size_t frame_at, int y0, int lane)
{
    if (lane < 30) {
        // row y0 + lane / 10 (the last run of a frame touches two: row 191 is then staged twice), bytes 4 j .. 4 j + 3 of its 40
        const int r = lane / 10, j = lane - 10 * r;
        const int y = min(y0 + r, 191);
        const size_t at = frame_at + (size_t)(render_row_offset(y) + 4 * j);
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
}

// unit g (0 .. 34) of a staged row: bit k is dot 16 g - 3 + k, k = 0 .. 18 (dots left of the row are 0)
__device__ static inline uint32_t render_unit_dots(const uint8_t *row, int g)
{
    // byte b of the staged row holds dots 7 b .. 7 b + 6; the unit shows dots 16 g .. 16 g + 15 and looks at three more
    // to their left: four bytes from bf = floor((16 g - 3) / 7) (-1 for g = 0: the zero byte in front of the row)
    const int bf = (16 * g + 4) / 7 - 1;
    const uint8_t *p = &row[8 + bf];
    const uint32_t mis = (uint32_t)(8 + bf) & 3u;
    const uint32_t *two = reinterpret_cast<const uint32_t *>(p - mis);   // (4-aligned only: two dword reads)
    const uint32_t v = __builtin_amdgcn_alignbyte(two[1], two[0], mis);
    const uint32_t d28 = (v & 0x7fu) | ((v >> 1) & 0x3f80u) | ((v >> 2) & 0x1fc000u) | ((v >> 3) & 0xfe00000u);
    return d28 >> (uint32_t)(16 * g - 3 - 7 * bf);
}

}  // namespace iiv
