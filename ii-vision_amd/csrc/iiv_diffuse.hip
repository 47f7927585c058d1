// iiv_diffuse.hip -- RGB frames -> HGR / DHGR memory maps by error diffusion with a CHOSEN kernel
// (include/iivision.h: iiv_frames_to_memory_maps_diffused): three rows of five weights over a divisor -- Floyd-Steinberg,
// Jarvis, Stucki, Atkinson, Burkes, the Sierras, bmp2dhr's "Buckels" (transcoder/frame_grabber.py: DIFFUSION_KERNELS).
//
// The shape is ingest_diffusion_kernel's (iiv_ingest.hip, which stays as it is: this entry point ALWAYS runs the kernel below,
// for Floyd-Steinberg's weights too, so that the two can be held against each other): lanes are rows, three frames of twenty
// rows per wave, a row SEVEN pixels behind the row above, hand-down by one wave-wide DPP shift, lane 19 -> lane 0 of the next
// pass through an LDS ring, the source rows through LDS by LDS-DMA, no barrier per pixel.  What differs is the reach:
//   * a pixel's error goes two pixels right, and two rows down, two pixels to either side.  Row r receives from rows r - 1
//     and r - 2, and a lane passes down TWO sums per channel and pixel j:
//         A(j) = sum_dx w[1][dx] e(j - dx) + B'(j)     what the row below adds to its own accumulator
//         B(j) = sum_dx w[2][dx] e(j - dx)             what the row below forwards: it is the B'(j) of ITS A(j)
//     (B' = the B received from the row above).  Both are final once pixel j + 2 of the sending row is done, so what a lane
//     receives at the start of its step for pixel p is (A, B)(p + 4): one pixel ahead of the farthest look HGR's palette-bit
//     decision takes (three pixels).  A waits in a seven-slot queue (slot = pixel mod 7) for its pixel, B for the step that
//     emits its pixel, six steps after it arrived.
//   * a sum is built as it becomes known: F(q) = w[.][0] e(q) + w[.][+1] e(q - 1) + w[.][+2] e(q - 2) at pixel q,
//     G(q) = F(q - 1) + w[.][-1] e(q), emitted(q) = G(q - 1) + w[.][-2] e(q) = the sum for pixel q - 2.  At a row's first and
//     second pixel the emitted sums are the last two of the FINISHED row: the new row's errors stay out of them (two selects),
//     and the finished row's stay out of the new row's because the same-row history restarts at zero.
//   * the same-row shares (w[0][+1], w[0][+2]) are added when the pixel is quantised; HGR's look-ahead adds w[0][+2] e(p - 1)
//     to pixel p + 1, the one same-row share that exists by then.
//   * floor(acc / divisor) is a 24-bit multiply and a shift: |acc| <= 255 x 64 (the weights sum to at most the divisor, the
//     divisor is at most 64), so (acc + bias) is below 2^15 and ((acc + bias) * M) >> s - bias / divisor is exact for
//     s = 15 + ceil(log2 divisor), M = ceil(2^s / divisor): checked here for every divisor over the whole range before the
//     first launch (div_table), and in tests/test_diffusion_model.py.
// Integer sums commute, so the schedule changes nothing: the result is the raster-order definition bit for bit.
// The palette's linear forms, the arg-min over them, mean_of and the screen-hole launch are
// iiv_frontend.h's, shared with iiv_ingest.hip; both files' kernels compile to the instructions they had with a copy each
// (profiles/frontend_isa_identity.txt).  The staged source stream below is still spelt here as it is there: as one shared
// type it did not compile to the same code (the same record).
#include "iiv_frontend.h"
#include "iiv_host.h"
#include "iiv_stream.h"
#include <type_traits>

namespace iiv {
namespace diffuse {

// The palette as the kernel takes it: the linear forms alone.  (A type of its own name: the kernel's symbol carries it.)
struct Palette : PaletteForms {};

// The diffusion kernel as the device kernel takes it: wave-uniform, by value
struct Weights {
    int32_t r1, r2;       // row 0: dx +1, +2
    int32_t w1[5], w2[5]; // rows 1 and 2: dx -2 .. +2
    uint32_t mul, shift;  // floor(acc / divisor) = (int)(((acc + bias) * mul) >> shift) - bias_q
    int32_t bias, bias_q; // bias = divisor * bias_q >= 255 * 64
};

constexpr int kAccMax = 255 * 64;
struct DivTable {
    uint32_t mul[65], shift[65];
    int32_t bias[65], bias_q[65];
    bool exact;
};
static DivTable make_div_table()
{
    DivTable t{};
    t.exact = true;
    for (int d = 1; d <= 64; d++) {
        uint32_t lg = 0;
        while ((1u << lg) < (uint32_t)d) lg++;
        t.shift[d] = 15 + lg;
        t.mul[d] = ((1u << t.shift[d]) + (uint32_t)d - 1) / (uint32_t)d;
        t.bias_q[d] = (kAccMax + d - 1) / d;
        t.bias[d] = t.bias_q[d] * d;
        for (int acc = -kAccMax; acc <= kAccMax; acc++) {
            const uint32_t a = (uint32_t)(acc + t.bias[d]);
            const int want = acc >= 0 ? acc / d : -((-acc + d - 1) / d);
            // (the device multiplies 24 bits by 24 bits and keeps the product's low 32)
            if (a >= (1u << 15) || t.mul[d] >= (1u << 24) || (uint64_t)a * t.mul[d] >= (1ull << 32) ||
                (int)((a * t.mul[d]) >> t.shift[d]) - t.bias_q[d] != want)
                t.exact = false;
        }
    }
    return t;
}

constexpr int kWaves = 2;        // waves per block
constexpr int kRows = 20;        // rows of a frame a wave works on at a time: 19 x 7 = 133 < 140, a lane goes on to row r + 20 without waiting
constexpr int kFrames = 3;       // frames per wave: 3 x 20 lanes, 4 idle
constexpr int kRingSlots = 8;    // the ring is written one step before it is read

// Geometry, source staging and the stores: ingest_diffusion_kernel's (iiv_ingest.hip), where they are explained.
template <int MODE>
__global__ __launch_bounds__(64 * kWaves, 3) void ingest_diffused_kernel(int n, const uint8_t *__restrict__ rgb_frames, const Palette P, const Weights W,
                                                                        uint8_t *__restrict__ main_mem, uint8_t *__restrict__ aux_mem)
{
    __shared__ int ring_s[kWaves][kFrames][kRingSlots][8];   // [A r g b, B r g b, -, -]
    __shared__ __attribute__((aligned(16))) uint32_t stage_s[kWaves][12][64][4];   // [slot x 4 + chunk][lane][16 B]
    __shared__ uint32_t pal_s[16];    // DHGR: R | G << 8 | B << 16 of the sixteen colour values
    __shared__ uint32_t rgb_s[8];     // R | G << 8 | B << 16 of colour4[pb][pattern]: black, violet | blue, green | orange, white
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x < 8) {
        constexpr int colour4[8] = {0, 3, 12, 15, 0, 6, 9, 15};
        rgb_s[threadIdx.x] = P.rgb[colour4[threadIdx.x]];
    }
    if (threadIdx.x < 16) pal_s[threadIdx.x] = P.rgb[threadIdx.x];
    __syncthreads();
    const int slot3 = lane / kRows, i = lane - kRows * slot3;    // frame slot 0..2 (3: idle lanes 60..63), row in the pass
    const size_t f = ((size_t)blockIdx.x * kWaves + wv) * kFrames + (size_t)(slot3 < kFrames ? slot3 : 0);
    const bool lane_ok = slot3 < kFrames && f < (size_t)n;
    int (*ring)[8] = ring_s[wv][slot3 < kFrames ? slot3 : 0];
    const uint8_t *frame = rgb_frames + (lane_ok ? f : 0) * (size_t)(192 * 280 * 3);
    const Kv kv = MODE == kDHGR ? kv_of(P) : Kv{};
    // HGR: the six colours it can show, their K in vector registers (iiv_frontend.h: Kv)
    int kv0 = P.k[0], kv3 = P.k[3], kv12 = P.k[12], kv15 = P.k[15], kv6 = P.k[6], kv9 = P.k[9];
    asm volatile("" : "+v"(kv0), "+v"(kv3), "+v"(kv12), "+v"(kv15), "+v"(kv6), "+v"(kv9));
    struct F6 {
        int f0, f3, f12, f15, f6, f9;
    };
    auto f6 = [&](int r, int g, int b) -> F6 {   // the distance terms of the six colours (dist_key)
        const v2s gb = __builtin_bit_cast(v2s, (uint32_t)g | ((uint32_t)b << 16));
        return F6{dist_key(P, kv0, 0, r, gb) >> 4, dist_key(P, kv3, 3, r, gb) >> 4, dist_key(P, kv12, 12, r, gb) >> 4,
                  dist_key(P, kv15, 15, r, gb) >> 4, dist_key(P, kv6, 6, r, gb) >> 4, dist_key(P, kv9, 9, r, gb) >> 4};
    };
    // per-lane sequence: group tt = T - i of this lane's rows (20 groups of 7 pixels per row; rows i, 20 + i, ...)
    int Aq[7][3], Bq[7][3];               // (A, B) from the row above for the pixels of the period, slot = pixel mod 7
#pragma unroll
    for (int j = 0; j < 7; j++) Aq[j][0] = Aq[j][1] = Aq[j][2] = Bq[j][0] = Bq[j][1] = Bq[j][2] = 0;
    int inA[3] = {0, 0, 0}, inB[3] = {0, 0, 0};   // what arrived at the end of the previous step: (A, B)(pixel + 4)
    int z1[3] = {0, 0, 0}, z2[3] = {0, 0, 0};     // errors of the previous two pixels of the row (0 in front of a row)
    int F1[3] = {0, 0, 0}, G1[3] = {0, 0, 0};     // the sums for the row below as they build up (see the top of the file)
    int F2[3] = {0, 0, 0}, G2[3] = {0, 0, 0};     // the same for the row after it
    uint32_t cur[11], nxt[11];            // the source bytes of the current / next 7-pixel group, funnel-shifted to start at byte 0
    int pbA = 0, pbB = 0;
    uint32_t bytesAB = 0;                 // HGR: the two screen bytes of the group, as they fill; DHGR: its 28 dots
    auto quot = [&](int acc) -> int {     // floor(acc / divisor), |acc| <= 255 x 64
        return (int)(__umul24((uint32_t)(acc + W.bias), W.mul) >> W.shift) - W.bias_q;
    };
    auto value_of = [&](uint32_t m, int ar, int ag, int ab, int &r, int &g, int &b) {   // clamp(mean + floor(acc / divisor))
        r = min(max((int)(m & 255u) + quot(ar), 0), 255);
        g = min(max((int)((m >> 8) & 255u) + quot(ag), 0), 255);
        b = min(max((int)((m >> 16) & 255u) + quot(ab), 0), 255);
    };
    int tt = -i;                          // this lane's group number at outer iteration T
    bool active = false, row_start = true;
    int row = i;
    size_t outp = 0;
    // ---- the staged source stream of this lane (byte offsets are relative to its frame; blocks = 64 bytes)
    uint32_t (*stage)[64][4] = stage_s[wv];
    const int last_pass_row = 180 + i < 192 ? 180 + i : 160 + i;   // this lane's last row
    int rd_row = i, rd_off = i * 840, rd_slot = 0;
    auto blocks_of_row = [](int rw) -> int { return ((rw * 840 + 839) >> 6) - ((rw * 840) >> 6) + 1; };
    int fe_row = i, fe_off = (i * 840) & ~63, fe_left = blocks_of_row(i), fe_slot = 0, fe_need = 3;
    auto fetch_round = [&]() {
        // every lane that still needs a block requests its next one: the lanes aiming at the same slot together
#pragma unroll
        for (int sl = 0; sl < 3; sl++) {
            const bool go = fe_need > 0 && fe_slot == sl;
            if (__ballot(go) == 0ull) continue;
            if (go) {
                const uint8_t *src = frame + fe_off;
#pragma unroll
                for (int c = 0; c < 4; c++) __builtin_amdgcn_global_load_lds(src + 16 * c, &stage[sl * 4 + c][0][0], 16, 0, 0);
                fe_need--;
                fe_slot = fe_slot == 2 ? 0 : fe_slot + 1;
                if (--fe_left == 0) {
                    fe_row = fe_row + kRows <= last_pass_row ? fe_row + kRows : fe_row;   // (behind its last row a lane reads that row again: never used)
                    fe_off = (fe_row * 840) & ~63;
                    fe_left = blocks_of_row(fe_row);
                } else {
                    fe_off += 64;
                }
            }
        }
    };
    auto read_group = [&](uint32_t (&w)[11]) {
        const int o = rd_off & 63;                        // the start inside its block (even)
        const int nx_slot = rd_slot == 2 ? 0 : rd_slot + 1;
        uint32_t D[16];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int t = (o & ~15) + 16 * k;             // chunk k of the window: byte offset from the block's start (< 128)
            const int sl = t < 64 ? rd_slot : nx_slot;
            const uint4 v = *reinterpret_cast<const uint4 *>(&stage[sl * 4 + ((t >> 4) & 3)][lane][0]);
            D[4 * k] = v.x, D[4 * k + 1] = v.y, D[4 * k + 2] = v.z, D[4 * k + 3] = v.w;
        }
        // (bitwise selects on opaque masks: a dynamic index would send the sixteen dwords through scratch)
        uint32_t m2 = 0u - (((uint32_t)o >> 3) & 1u), m1 = 0u - (((uint32_t)o >> 2) & 1u);
        asm volatile("" : "+v"(m2), "+v"(m1));
        uint32_t E[14], F[12];
#pragma unroll
        for (int j = 0; j < 14; j++) E[j] = (D[j + 2] & m2) | (D[j] & ~m2);   // v_bfi_b32
#pragma unroll
        for (int j = 0; j < 12; j++) F[j] = (E[j + 1] & m1) | (E[j] & ~m1);
        const uint32_t sh = ((uint32_t)o & 2u) * 8u;
#pragma unroll
        for (int j = 0; j < 10; j++) w[j] = __builtin_amdgcn_alignbit(F[j + 1], F[j], sh);
        w[10] = F[10] >> sh;
    };
    // the reader moves on to group g (>= 1) of this lane's sequence; the blocks it leaves behind become requests
    auto advance_reader = [&](int g) {
        if (g < 1) return;                                // (in front of its first group a lane reads group 0 again and again)
        const int gg = g % 20, rw = kRows * (g / 20) + i;
        if (rw > last_pass_row) return;                   // (behind its last row: it stays where it is; nothing of it is used)
        const int old_blk = rd_off >> 6;
        int d;
        if (gg == 0) {                                    // a new row: the rest of the old row's blocks, then the new row's first
            const int old_last = (rd_row * 840 + 839) >> 6;
            d = old_last - old_blk + 1;
            rd_row = rw;
            rd_off = rw * 840;
        } else {
            rd_off += 42;
            d = (rd_off >> 6) - old_blk;
        }
        rd_slot = rd_slot + d;
        rd_slot = rd_slot >= 3 ? rd_slot - 3 : rd_slot;
        fe_need += d;
    };
    auto staged_wait = []() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
    fetch_round();
    fetch_round();
    fetch_round();
    staged_wait();
    read_group(cur);
    advance_reader(tt + 1);
    fetch_round();
    fetch_round();
    staged_wait();
    read_group(nxt);
    advance_reader(tt + 2);
    fetch_round();
    fetch_round();
    auto step = [&](auto Pc) {
        constexpr int PH = decltype(Pc)::value;
        // what arrived: (A, B)(pixel + 4) of the row above, into its slots; lane 0 of a frame slot takes it from the ring
        {
            const int s = 7 * tt + PH - 136;         // lane 19's sequence index of it
            const int *slot = ring[s & (kRingSlots - 1)];
            int s0 = slot[0], s1 = slot[1], s2 = slot[2], s3 = slot[3], s4 = slot[4], s5 = slot[5];
            asm volatile("" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3), "+v"(s4), "+v"(s5));   // (read by every lane: kept out of an exec region each)
            const bool from_ring = i == 0, has = s >= 0;
            constexpr int Q = (PH + 4) % 7;
            Aq[Q][0] = from_ring ? (has ? s0 : 0) : inA[0];
            Aq[Q][1] = from_ring ? (has ? s1 : 0) : inA[1];
            Aq[Q][2] = from_ring ? (has ? s2 : 0) : inA[2];
            Bq[Q][0] = from_ring ? (has ? s3 : 0) : inB[0];
            Bq[Q][1] = from_ring ? (has ? s4 : 0) : inB[1];
            Bq[Q][2] = from_ring ? (has ? s5 : 0) : inB[2];
        }
        int e[3] = {0, 0, 0};
        if (active) {
            int r, g, b;
            value_of(mean_of<PH>(cur), Aq[PH][0] + __mul24(W.r1, z1[0]) + __mul24(W.r2, z2[0]), Aq[PH][1] + __mul24(W.r1, z1[1]) + __mul24(W.r2, z2[1]),
                     Aq[PH][2] + __mul24(W.r1, z1[2]) + __mul24(W.r2, z2[2]), r, g, b);
            if constexpr (MODE == kDHGR) {
                // the nearest of the sixteen colours; its value IS the pixel's dot quad
                const int col = nearest16_mad(P, kv, r, g, b);
                const uint32_t prgb = pal_s[col];
                e[0] = r - (int)(prgb & 255u);
                e[1] = g - (int)((prgb >> 8) & 255u);
                e[2] = b - (int)((prgb >> 16) & 255u);
                bytesAB |= (uint32_t)col << (4 * PH);
                if (PH == 6) {
                    const uint32_t b0 = bytesAB & 0x7fu, b1 = (bytesAB >> 7) & 0x7fu, b2 = (bytesAB >> 14) & 0x7fu, b3 = (bytesAB >> 21) & 0x7fu;
                    *reinterpret_cast<uint16_t *>(aux_mem + outp) = (uint16_t)(b0 | (b2 << 8));
                    *reinterpret_cast<uint16_t *>(main_mem + outp) = (uint16_t)(b1 | (b3 << 8));
                    outp += 2;
                    bytesAB = 0;
                }
            } else {
                const F6 fk = f6(r, g, b);
                if (PH == 0 || PH == 4) {
                    // the palette bit of the byte this pixel opens: summed nearest-colour errors of the pixels that start in it
                    // (weights: their dots in the byte; the term common to all colours cancels), ties to 0.  A pixel ahead has
                    // what the rows above sent it and, the next one, the previous pixel's share two to the right.
                    int s0 = 2 * min(min(fk.f0, fk.f3), min(fk.f12, fk.f15)), s1 = 2 * min(min(fk.f0, fk.f6), min(fk.f9, fk.f15));
                    auto ahead = [&](auto Qc, int w) {
                        constexpr int Q = decltype(Qc)::value;
                        int r2, g2, b2;
                        if (Q == PH + 1)
                            value_of(mean_of<Q>(cur), Aq[Q][0] + __mul24(W.r2, z1[0]), Aq[Q][1] + __mul24(W.r2, z1[1]), Aq[Q][2] + __mul24(W.r2, z1[2]), r2, g2, b2);
                        else
                            value_of(mean_of<Q>(cur), Aq[Q][0], Aq[Q][1], Aq[Q][2], r2, g2, b2);
                        const F6 fa = f6(r2, g2, b2);
                        s0 += __mul24(w, min(min(fa.f0, fa.f3), min(fa.f12, fa.f15)));   // (|f| < 2^21)
                        s1 += __mul24(w, min(min(fa.f0, fa.f6), min(fa.f9, fa.f15)));
                    };
                    if (PH == 0) {
                        ahead(std::integral_constant<int, 1>{}, 2);
                        ahead(std::integral_constant<int, 2>{}, 2);
                        ahead(std::integral_constant<int, 3>{}, 1);
                        pbA = s1 < s0 ? 1 : 0;
                    } else {
                        ahead(std::integral_constant<int, 5>{}, 2);
                        ahead(std::integral_constant<int, 6>{}, 2);
                        pbB = s1 < s0 ? 1 : 0;
                    }
                }
                const int pb = PH < 4 ? pbA : pbB;
                const int k0 = min(min(fk.f0 * 4, fk.f3 * 4 + 1), min(fk.f12 * 4 + 2, fk.f15 * 4 + 3));
                const int k1 = min(min(fk.f0 * 4, fk.f6 * 4 + 1), min(fk.f9 * 4 + 2, fk.f15 * 4 + 3));
                const uint32_t pat = (uint32_t)(pb ? k1 : k0) & 3u;
                const uint32_t prgb = rgb_s[pb * 4 + (int)pat];
                e[0] = r - (int)(prgb & 255u);
                e[1] = g - (int)((prgb >> 8) & 255u);
                e[2] = b - (int)((prgb >> 16) & 255u);
                // dots 2 PH, 2 PH + 1 of the group: byte A = dots 0..6 | palette bit, byte B = dots 7..13 | palette bit
                if (PH < 3) bytesAB |= pat << (2 * PH);
                if (PH == 3) bytesAB |= ((pat & 1u) << 6) | ((uint32_t)pbA << 7) | ((pat >> 1) << 8);
                if (PH > 3) bytesAB |= pat << (2 * PH + 1);       // PH 4, 5, 6 -> bits 9, 11, 13 (byte B bits 1, 3, 5)
                if (PH == 6) {
                    *reinterpret_cast<uint16_t *>(main_mem + outp) = (uint16_t)(bytesAB | ((uint32_t)pbB << 15));
                    outp += 2;
                    bytesAB = 0;
                }
            }
        }
        // to the row below: the sums for pixel (this pixel - 2) -- at a row's first two pixels, and behind a lane's last row,
        // pixels 138 and 139 of the finished row, which the new row's errors stay out of
        int outA[3], outB[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int eG = (PH == 0 && row_start) ? 0 : e[c];
            const int eO = (PH <= 1 && row_start) ? 0 : e[c];
            outA[c] = G1[c] + __mul24(W.w1[0], eO) + Bq[(PH + 5) % 7][c];
            outB[c] = G2[c] + __mul24(W.w2[0], eO);
            G1[c] = F1[c] + __mul24(W.w1[1], eG);
            G2[c] = F2[c] + __mul24(W.w2[1], eG);
            F1[c] = __mul24(W.w1[2], e[c]) + __mul24(W.w1[3], z1[c]) + __mul24(W.w1[4], z2[c]);
            F2[c] = __mul24(W.w2[2], e[c]) + __mul24(W.w2[3], z1[c]) + __mul24(W.w2[4], z2[c]);
            z2[c] = z1[c];
            z1[c] = e[c];
        }
        {
            const int s = 7 * tt + PH - 2;            // this lane's sequence index of what it emits
            if (i == kRows - 1 && s >= 0) {
                int *slot = ring[s & (kRingSlots - 1)];
                slot[0] = outA[0], slot[1] = outA[1], slot[2] = outA[2];
                slot[3] = outB[0], slot[4] = outB[1], slot[5] = outB[2];
            }
        }
        wave_lds_sync();
#pragma unroll
        for (int c = 0; c < 3; c++) {
            inA[c] = __builtin_amdgcn_update_dpp(0, outA[c], 0x138, 0xf, 0xf, false);   // wave_shr:1
            inB[c] = __builtin_amdgcn_update_dpp(0, outB[c], 0x138, 0xf, 0xf, false);
        }
    };
    // lane i starts at T = i and runs 200 groups (pass 9: rows 180 + i < 192 only); one more iteration flushes the last rows
    for (int T = 0; T < kRows - 1 + 200 + 1; T++) {
        const int qq = tt >= 0 ? tt / 20 : 0;
        row = kRows * qq + i;
        active = lane_ok && tt >= 0 && row < 192;
        row_start = tt % 20 == 0 || !active;
        if (tt >= 0 && tt % 20 == 0) {
            // a new row: nothing from the left; where its bytes go
#pragma unroll
            for (int c = 0; c < 3; c++) z1[c] = z2[c] = 0;
            outp = f * 8192 + (size_t)y_to_offset(row < 192 ? row : 191);
        }
        step(std::integral_constant<int, 0>{});
        step(std::integral_constant<int, 1>{});
        step(std::integral_constant<int, 2>{});
        step(std::integral_constant<int, 3>{});
        step(std::integral_constant<int, 4>{});
        step(std::integral_constant<int, 5>{});
        // what was requested at the end of the previous iteration has landed by now (six steps later).  HERE, not at the read
        // below: behind step 6 the wait would also cover the row's stores that step has just issued
        staged_wait();
        step(std::integral_constant<int, 6>{});
#pragma unroll
        for (int j = 0; j < 11; j++) cur[j] = nxt[j];
        tt++;
        read_group(nxt);          // group tt + 1: where the reader stands (its blocks: waited for in front of step 6)
        advance_reader(tt + 2);
        fetch_round();            // the blocks left behind: at most two per lane (a row's end)
        if (__ballot(fe_need > 0) != 0ull) fetch_round();
    }
}

static int frames_to_memory_maps_diffused(int mode, const uint8_t palette_rgb[48], int n, const uint8_t *d_rgb, const Weights &W,
                                          uint8_t *d_main, uint8_t *d_aux, hipStream_t st)
{
    const Palette P{make_palette_forms(palette_rgb)};
    if (int rc = zero_screen_holes(mode, n, d_main, d_aux, st)) return rc;
    const dim3 grid((unsigned)((n + kFrames * kWaves - 1) / (kFrames * kWaves)));
    return launch(by_mode(mode, ingest_diffused_kernel<kDHGR>, ingest_diffused_kernel<kHGR>), "ingest_diffused_kernel launch", grid,
                  dim3(64 * kWaves), 0, st, n, d_rgb, P, W, d_main, d_aux);
}

}  // namespace diffuse
}  // namespace iiv

extern "C" int iiv_frames_to_memory_maps_diffused(int mode, const uint8_t palette_rgb[48], int n_frames, const uint8_t *d_rgb,
                                                  const uint8_t weights[15], int divisor, uint8_t *d_main, uint8_t *d_aux,
                                                  void *stream)
{
    using namespace iiv::diffuse;
    if ((mode != IIV_HGR && mode != IIV_DHGR) || !palette_rgb || n_frames < 0 || !d_rgb || !d_main || (mode == IIV_DHGR && !d_aux) ||
        !weights)
        return iiv::set_error(IIV_ERR_INVALID, "iiv_frames_to_memory_maps_diffused: bad argument");
    if (((uintptr_t)d_rgb & 3) || ((uintptr_t)d_main & 7) || ((uintptr_t)d_aux & 7))
        return iiv::set_error(IIV_ERR_INVALID, "iiv_frames_to_memory_maps_diffused: d_rgb must be 4-byte aligned, d_main / d_aux 8-byte aligned");
    if (divisor < 1 || divisor > 64)
        return iiv::set_error(IIV_ERR_INVALID, "iiv_frames_to_memory_maps_diffused: divisor %d is outside 1..64", divisor);
    if (weights[0] || weights[1] || weights[2])
        return iiv::set_error(IIV_ERR_INVALID, "iiv_frames_to_memory_maps_diffused: weights[0..2] (the pixel itself and what lies left of it) must be 0");
    int sum = 0;
    for (int j = 0; j < 15; j++) sum += weights[j];
    if (sum > divisor)
        return iiv::set_error(IIV_ERR_INVALID, "iiv_frames_to_memory_maps_diffused: the weights sum to %d, more than the divisor %d", sum, divisor);
    static const DivTable div = make_div_table();
    if (!div.exact) return iiv::set_error(IIV_ERR_ASSERT, "iiv_frames_to_memory_maps_diffused: the multiply-and-shift division is not exact");
    if (n_frames == 0) return IIV_OK;
    Weights W;
    W.r1 = weights[3], W.r2 = weights[4];
    for (int j = 0; j < 5; j++) W.w1[j] = weights[5 + j], W.w2[j] = weights[10 + j];
    W.mul = div.mul[divisor], W.shift = div.shift[divisor], W.bias = div.bias[divisor], W.bias_q = div.bias_q[divisor];
    return frames_to_memory_maps_diffused(mode, palette_rgb, n_frames, d_rgb, W, d_main, d_aux, (hipStream_t)stream);
}
