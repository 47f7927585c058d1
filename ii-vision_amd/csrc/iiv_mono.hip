// iiv_mono.hip -- RGB frames -> HGR / DHGR memory maps for a MONOCHROME monitor on gfx950.
//
// On a mono screen a (D)HGR picture is W x 192 one-bit dots, W = 560 (DHGR) or 280 (HGR): the source frame has one pixel
// per dot, a dot is lit where the (dithered) luma reaches 128.  The conversion is specified, in integer arithmetic, in
// include/iivision.h (iiv_frames_to_memory_maps_mono); tests/mono_model.py restates it and the tests hold these kernels
// to that restatement byte for byte.
//   * Ordered dither: one thread per FOURTEEN dots = two screen bytes (DHGR: the aux and the main byte of a column;
//     HGR: two main bytes): its 42 source bytes are eleven aligned dword loads and a funnel shift (iiv_frontend.h:
//     load_group42, which ingest_kernel shares).  No dot is evaluated twice, nothing is exchanged.
//   * Error diffusion: lanes are ROWS, a wave is a frame.  Lane r works on rows r, 64 + r, 128 + r one after the other,
//     two dots behind lane r - 1: at step t it is at position s = t - 2 r of its 3 W dots.  What a row hands down,
//     D(j) = e(j - 1) + 5 e(j) + 3 e(j + 1), is final once dot j + 1 is done -- exactly one step before the lane below
//     needs it -- and moves there by one wave-wide DPP shift.  Row 64 b + 63 -> row 64 (b + 1) goes from lane 63 to lane 0
//     through one row of LDS: lane 63 writes D(j) at step b W + j + 127, lane 0 reads it at step (b + 1) W + j (W > 142:
//     always written long before, and not yet overwritten).  Integer sums commute, so the schedule changes nothing.
//     3 W + 126 steps per frame.
//   * The diffusion does not read RGB: a pre-pass writes the luma as bytes in the order the diffusion reads them -- the
//     sixteen steps 16 k .. 16 k + 15 of lane r are the uint4 at (k * 64 + r): one dwordx4 load per lane and sixteen
//     steps, 1 KiB contiguous per wave (sixty-four lanes walking sixty-four rows would touch sixty-four cache lines per
//     load: what bound the colour kernel).  The pre-pass writes into stream-ordered scratch, a chunk of
//     frames at a time.
#include "iiv_frontend.h"
#include "iiv_host.h"
#include <stdlib.h>

namespace iiv {
namespace {

template <int MODE> struct MonoGeom {
    static constexpr int W = MODE == kDHGR ? 560 : 280;          // dots per row = source pixels per row
    static constexpr int kRowBytes = W / 7;                      // screen bytes per row (DHGR: both banks)
    static constexpr int kFrameBytes = 192 * W * 3;              // source bytes per frame (a multiple of 4)
    static constexpr int kSteps = 3 * W + 126;                   // diffusion steps of a frame
    static constexpr int kGroups = (kSteps + 15) / 16;           // 16-step groups
    static constexpr size_t kSkewBytes = (size_t)kGroups * 64 * 16;   // luma scratch per frame
};

struct MonoDither {
    int32_t d[16];   // ordered-dither offset of (y & 3) * 4 + (x & 3): floor((2 Bayer - 15) * amplitude / 16)
};

MonoDither make_dither(int dither)
{
    MonoDither p;
    dither_offsets(dither, p.d);
    return p;
}

__device__ inline int mono_luma(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }

// Ordered dither (or none): thread T of a frame owns dots 14 g .. 14 g + 13 of row y, T = (W / 14) y + g -- the frame's
// source bytes are 42 contiguous bytes per thread in thread order.  (Eleven dwords from the aligned base never leave the
// frame: a group at an odd halfword -- every odd T, the frame's last among them -- ends with its eleventh dword.)
template <int MODE>
__global__ __launch_bounds__(256) void mono_ordered_kernel(int n, const uint8_t *__restrict__ rgb_frames, const MonoDither P,
                                                           uint8_t *__restrict__ main_mem, uint8_t *__restrict__ aux_mem)
{
    using G = MonoGeom<MODE>;
    constexpr int TPR = G::W / 14, TPF = 192 * TPR;
    __shared__ int dtab[16];
    if (threadIdx.x < 16) dtab[threadIdx.x] = P.d[threadIdx.x];
    __syncthreads();
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * TPF) return;
    const size_t f = idx / TPF;
    const int T = (int)(idx - f * TPF), y = T / TPR, g = T - TPR * y;
    SourceBytes<11> src;   // the 42 bytes at 42 T
    load_group42(rgb_frames + f * (size_t)G::kFrameBytes, 42 * T, src.q);
    const int drow = (y & 3) * 4;
    uint32_t dots = 0;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        const int d = dtab[drow + ((14 * g + i) & 3)];
        const int v = min(max(mono_luma(src.byte_at(3 * i), src.byte_at(3 * i + 1), src.byte_at(3 * i + 2)) + d, 0), 255);
        dots |= (uint32_t)(v >= 128 ? 1 : 0) << i;
    }
    const uint32_t A = dots & 0x7fu, B = (dots >> 7) & 0x7fu;   // bytes 2 g and 2 g + 1 of the row
    if (MODE == kDHGR) {
        // even bytes of the row's 80 -> aux, odd -> main, column X / 14 (screen.py:822-826)
        const size_t out = f * 8192 + (size_t)(y_to_offset(y) + g);
        aux_mem[out] = (uint8_t)A;
        main_mem[out] = (uint8_t)B;
    } else {
        const size_t out = f * 8192 + (size_t)(y_to_offset(y) + 2 * g);
        *reinterpret_cast<uint16_t *>(main_mem + out) = (uint16_t)(A | (B << 8));
    }
}

// The luma of n frames in the diffusion's order: thread (f, k, r) writes the uint4 of lane r's steps 16 k .. 16 k + 15,
// positions s = 16 k - 2 r + i of the lane's 3 W dots: row r + 64 (s / W), dot s % W; zero outside 0 .. 3 W - 1.
// A group inside one row (all but a handful per lane) is 48 contiguous source bytes at an even offset: twelve or thirteen
// aligned dwords and a funnel shift.  (The thirteenth is read only at an odd halfword; the bytes behind such a group's
// 48 are then inside the frame -- its size is a multiple of four.)
template <int MODE>
__global__ __launch_bounds__(256) void mono_luma_skew_kernel(int n, const uint8_t *__restrict__ rgb_frames, uint4 *__restrict__ skew)
{
    using G = MonoGeom<MODE>;
    constexpr int W = G::W;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * G::kGroups * 64) return;
    const size_t f = idx / (G::kGroups * 64);
    const int rem = (int)(idx - f * (G::kGroups * 64)), k = rem >> 6, r = rem & 63;
    const uint8_t *frame = rgb_frames + f * (size_t)G::kFrameBytes;
    const int s0 = 16 * k - 2 * r;
    uint32_t o[4] = {0, 0, 0, 0};
    if (s0 >= 0 && s0 + 15 < 3 * W && s0 / W == (s0 + 15) / W) {
        const int band = s0 / W, x0 = s0 - band * W;
        const int off = ((r + 64 * band) * W + x0) * 3;
        const uint32_t *p = reinterpret_cast<const uint32_t *>(frame + (off & ~3));
        const uint32_t sh = ((uint32_t)off & 2u) * 8u;
        uint32_t w[13];
#pragma unroll
        for (int j = 0; j < 12; j++) w[j] = p[j];
        w[12] = sh ? p[12] : 0u;
        SourceBytes<12> src;
#pragma unroll
        for (int j = 0; j < 12; j++) src.q[j] = __builtin_amdgcn_alignbit(w[j + 1], w[j], sh);
#pragma unroll
        for (int i = 0; i < 16; i++)
            o[i >> 2] |= (uint32_t)mono_luma(src.byte_at(3 * i), src.byte_at(3 * i + 1), src.byte_at(3 * i + 2)) << (8 * (i & 3));
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int s = s0 + i;
            if (s >= 0 && s < 3 * W) {
                const int band = s / W, x = s - band * W;
                const uint8_t *p = frame + ((r + 64 * band) * W + x) * 3;
                o[i >> 2] |= (uint32_t)mono_luma(p[0], p[1], p[2]) << (8 * (i & 3));
            }
        }
    }
    skew[idx] = make_uint4(o[0], o[1], o[2], o[3]);
}

// dither == IIV_DITHER_DIFFUSION: Floyd-Steinberg over the W x 192 dots (the schedule: top of this file).
constexpr int kMonoWaves = 4;   // waves (= frames) per block
template <int MODE>
__global__ __launch_bounds__(64 * kMonoWaves) void mono_diffusion_kernel(int n, const uint4 *__restrict__ skew, uint8_t *__restrict__ main_mem,
                                                                         uint8_t *__restrict__ aux_mem)
{
    using G = MonoGeom<MODE>;
    constexpr int W = G::W;
    __shared__ int rowbuf_s[kMonoWaves][W];   // D(0 .. W - 1) of the last row of the band above: lane 63 -> lane 0
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t f = (size_t)blockIdx.x * kMonoWaves + wv;
    if (f >= (size_t)n) return;               // (a whole wave; no workgroup barrier below)
    int *rb = rowbuf_s[wv];
    for (int j = lane; j < W; j += 64) rb[j] = 0;   // band 0 has no row above: lane 0 reads these before lane 63 writes
    const uint4 *src = skew + f * (size_t)(G::kGroups * 64) + lane;
    uint8_t *out_main = main_mem + f * 8192, *out_aux = MODE == kDHGR ? aux_mem + f * 8192 : nullptr;
    uint4 nxt = src[0];
    int e1 = 0;              // error of the previous dot of the row
    int h = 0;               // e(x - 2) + 5 e(x - 1)
    int in = 0;              // what arrived from the lane above at the end of the previous step: D(x) of the row above
    int s = -2 * lane;       // this lane's position in its 3 W dots
    uint32_t bits = 0;       // dots not yet stored, oldest in bit 0
    int nb = 0;
    int orow = lane, ob = 0; // where the next stored byte goes: byte ob of row orow
    int xb = 0;              // lane 0's dot of the group's first step: 16 k mod W
    for (int k = 0; k < G::kGroups; k++) {
        const uint4 cur = nxt;
        nxt = src[(size_t)(k + 1 < G::kGroups ? k + 1 : k) * 64];
        const uint32_t yw[4] = {cur.x, cur.y, cur.z, cur.w};
        // lane 0's D from the row above for the sixteen steps (read by every lane: a uniform address is a broadcast)
        int rbv[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int j = xb + i;
            rbv[i] = rb[j >= W ? j - W : j];
        }
        xb = xb + 16 >= W ? xb + 16 - W : xb + 16;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int Y = (int)((yw[i >> 2] >> (8 * (i & 3))) & 255u);
            const bool act = s >= 0 && s < 3 * W;
            const int x = s - (s >= W ? W : 0) - (s >= 2 * W ? W : 0);   // (s = 3 W, the flush behind the last row: W)
            const bool first = x == 0;
            const int din = lane == 0 ? rbv[i] : in;
            const int el = first ? 0 : e1;                               // nothing from the left at a row's first dot
            // 7 e + D as (e << 3) + (D - e)
            const int v = min(max(Y + (((el << 3) + (din - el)) >> 4), 0), 255);
            const int dot = v >= 128 ? 1 : 0;
            const int e = v - (dot ? 255 : 0);
            // to the row below: D(x - 1) = e(x - 2) + 5 e(x - 1) + 3 e(x); at a row's first dot and behind the lane's last
            // row D(W - 1) of the finished row, which has no dot to its right
            int out = h;
            if (act) {
                if (!first) out += 3 * e;
                h = el + 5 * e;
                e1 = e;
                bits |= (uint32_t)dot << nb;
                nb++;
            } else {
                h = 0;
            }
            if (lane == 63 && s >= 0 && s <= 3 * W) rb[x == 0 ? W - 1 : x - 1] = out;
            in = __builtin_amdgcn_update_dpp(0, out, 0x138, 0xf, 0xf, false);   // wave_shr:1 (lane 0: 0)
            s++;
        }
        // whole bytes: at most three (6 left over + 16 new dots); a row is a whole number of bytes
#pragma unroll
        for (int j = 0; j < 3; j++) {
            if (nb >= 7) {
                const uint8_t b = (uint8_t)(bits & 0x7fu);
                if (MODE == kDHGR)
                    ((ob & 1) ? out_main : out_aux)[y_to_offset(orow) + (ob >> 1)] = b;
                else
                    out_main[y_to_offset(orow) + ob] = b;
                bits >>= 7;
                nb -= 7;
                if (++ob == G::kRowBytes) ob = 0, orow += 64;
            }
        }
    }
}

template <int MODE>
int mono_frames(int n, const uint8_t *d_rgb, int dither, uint8_t *d_main, uint8_t *d_aux, hipStream_t st)
{
    using G = MonoGeom<MODE>;
    if (dither != IIV_DITHER_DIFFUSION) {
        const MonoDither P = make_dither(dither);
        const size_t total = (size_t)n * 192 * (G::W / 14);
        return launch(mono_ordered_kernel<MODE>, "mono_ordered_kernel launch", dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, n,
                      d_rgb, P, d_main, d_aux);
    }
    // A wave is a frame and one wave alone issues an instruction every four cycles, so a chunk should put two waves on
    // each of the 1024 SIMDs -- and its luma, written and read once, should still be in the 256 MiB Infinity Cache when
    // the diffusion reads it: 2048 frames (226 MiB DHGR, 122 MiB HGR).  Measured, M DHGR frames/s by frames per chunk:
    // 256: 0.87, 1024: 2.52, 2048: 2.90, 4096: 2.25, 8192: 2.26 (profiles/mono_probe.txt).
    // (IIV_EXP_MONO_CHUNK: timing experiments only -- frames per chunk)
    static const int chunk_env = getenv("IIV_EXP_MONO_CHUNK") ? atoi(getenv("IIV_EXP_MONO_CHUNK")) : 0;
    int chunk = chunk_env > 0 ? chunk_env : 2048;
    if (chunk > n) chunk = n;
    uint4 *skew = nullptr;
    IIV_HIP(hipMallocAsync((void **)&skew, (size_t)chunk * G::kSkewBytes, st));
    int rc = 0;
    for (int f0 = 0; f0 < n && !rc; f0 += chunk) {
        const int fn = n - f0 < chunk ? n - f0 : chunk;
        const size_t items = (size_t)fn * G::kGroups * 64;
        rc = launch(mono_luma_skew_kernel<MODE>, "mono_luma_skew_kernel launch", dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, fn,
                    d_rgb + (size_t)f0 * G::kFrameBytes, skew);
        if (rc) break;
        rc = launch(mono_diffusion_kernel<MODE>, "mono_diffusion_kernel launch", dim3((unsigned)((fn + kMonoWaves - 1) / kMonoWaves)),
                    dim3(64 * kMonoWaves), 0, st, fn, skew, d_main + (size_t)f0 * 8192,
                    MODE == kDHGR ? d_aux + (size_t)f0 * 8192 : (uint8_t *)nullptr);
    }
    const int rc_free = hip_check(hipFreeAsync(skew, st), "hipFreeAsync(mono luma scratch)");
    return rc ? rc : rc_free;
}

}  // namespace
}  // namespace iiv

extern "C" int iiv_frames_to_memory_maps_mono(int mode, int n_frames, const uint8_t *d_rgb, int dither, uint8_t *d_main,
                                              uint8_t *d_aux, void *stream)
{
    if ((mode != IIV_HGR && mode != IIV_DHGR) || n_frames < 0 || !d_rgb || !d_main || (mode == IIV_DHGR && !d_aux) || dither < 0 ||
        dither > IIV_DITHER_DIFFUSION)
        return iiv::set_error(IIV_ERR_INVALID, "iiv_frames_to_memory_maps_mono: bad argument");
    if (((uintptr_t)d_rgb & 3) || ((uintptr_t)d_main & 7) || (mode == IIV_DHGR && ((uintptr_t)d_aux & 7)))
        return iiv::set_error(IIV_ERR_INVALID, "iiv_frames_to_memory_maps_mono: d_rgb must be 4-byte aligned, d_main / d_aux 8-byte aligned");
    if (n_frames == 0) return IIV_OK;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = iiv::zero_screen_holes(mode, n_frames, d_main, d_aux, st)) return rc;
    return mode == IIV_DHGR ? iiv::mono_frames<iiv::kDHGR>(n_frames, d_rgb, dither, d_main, d_aux, st)
                            : iiv::mono_frames<iiv::kHGR>(n_frames, d_rgb, dither, d_main, d_aux, st);
}
