// iiv_resize.hip -- source frames -> 280x192 (any H x W up to 1024) on gfx950, byte-exact with Pillow's
// Image.resize(..., LANCZOS): the step the reference applies to every decoded frame (frame_grabber.py:75,100).
//
// The contract (include/iivision.h: iiv_resize_coeffs / iiv_resize_frames):
//   * per axis, float64 Lanczos-3 weights per output sample, normalised and rounded to 22-bit fixed point -- computed
//     HERE ON THE HOST with libm sin, as Pillow computes them (a device sin may differ in the last ulp and flip a rounding);
//   * a pass is out = clamp((2^21 + sum(pixel * k)) >> 22, 0, 255) in int32, each channel on its own -- integer
//     multiply-adds only, so the order of the sum is free;
//   * the horizontal pass first (vertical first when h > 100 w), the first pass's uint8 result feeding the second; an axis
//     whose size does not change gets no pass.
//
// Form: two kernels, the first pass's uint8 result in a stream-ordered HBM scratch of frames_per_piece frames, sized so a
// chunk's intermediate (at most W / w of its source) stays in the Infinity Cache between the two launches.  Source
// bytes cross HBM once.
//   * resize_h_kernel<R, Rows>: a workgroup per R source rows, one thread per output column.  A row source unpacks the rows
//     to one dword per pixel in LDS; each tap is then one coalesced coefficient load (the table is stored tap-major), R LDS
//     reads and 3 R 24-bit multiply-adds.  Two row sources: RgbRows (packed RGB, aligned dword loads and a funnel shift, any
//     byte stride) and YuvRows (4:2:0 planes, iiv_resize_frames_yuv420: converted as they are unpacked).
//   * resize_v_kernel: a workgroup per output row, one thread per four bytes of the row (the vertical pass does not care
//     which byte is which channel); the row's coefficients are wave-uniform (scalar loads).
// One driver, resize_rows<Rows>, serves all entry points: tables, pass order, slices and chunks, scratch.  Coefficient tables
// are made once per (device, in, box, out) and kept for the life of the process.
// f12 (iiv_resize_frames_fit / iiv_resize_frames_yuv420_fit): a box of the source -- float32, as Pillow's
// Image.resize(box=) holds it -- goes into a rectangle of the destination and resize_fill_kernel gives the rest a fill colour.
// The same kernels and driver: a row source is a window of its frames, and only the columns and rows the tables touch are staged.
#include "iiv_host.h"

#include <math.h>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <vector>

namespace iiv {
namespace {

constexpr int kPrecisionBits = 22;
constexpr int kMaxIn = 8192, kMaxOut = 1024;
constexpr size_t kChunkMidBytes = 32u << 20;   // intermediate per chunk of frames (the Infinity Cache holds 256 MiB)

double sinc(double x)
{
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

double lanczos(double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3.0) : 0.0; }

// (f12: Pillow holds a box as float32 and subtracts in float32 before it widens; the whole axis is in0 = 0, in1 = in_size)
double scale_of(float in0, float in1, int out_size) { return (double)(in1 - in0) / out_size; }

int ksize_of(float in0, float in1, int out_size)
{
    double filterscale = scale_of(in0, in1, out_size);
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(3.0 * filterscale) * 2 + 1;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc over the box [in0, in1) of an axis of in_size samples: bounds [out][2] =
// (xmin, count), clamped at the AXIS, not at the box, coeffs [out][ksize], zero past count
void make_coeffs(int in_size, float in0, float in1, int out_size, int ksize, int32_t *bounds, int32_t *coeffs)
{
    const double scale = scale_of(in0, in1, out_size);
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * filterscale;
    const double ss = 1.0 / filterscale;
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out_size; xx++) {
        const double center = (double)in0 + (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; x++) {
            w[x] = lanczos((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t *k = coeffs + (size_t)xx * ksize;
        for (int x = 0; x < ksize; x++) {
            double v = x < xmax ? (ww != 0.0 ? w[x] / ww : w[x]) : 0.0;
            k[x] = v < 0 ? (int32_t)(v * (1 << kPrecisionBits) - 0.5) : (int32_t)(v * (1 << kPrecisionBits) + 0.5);
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

// one axis's tables on one device: bounds (xmin, count) per output sample, the coefficients out-major ([out][ksize]: the
// vertical pass reads one row's taps) and tap-major ([ksize][out]: the horizontal pass's lanes read consecutive outputs)
struct Table {
    int ksize = 0;
    int lo = 0, hi = 0;   // the input samples [lo, hi) that the bounds touch
    int2 *bounds = nullptr;
    int32_t *k_rows = nullptr, *k_taps = nullptr;
};

uint32_t bits_of(float v)
{
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}

int get_table(int in_size, float in0, float in1, int out_size, const Table **out)
{
    static std::mutex mu;
    static std::map<std::tuple<int, int, uint32_t, uint32_t, int>, Table> cache;
    int dev = 0;
    IIV_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto key = std::make_tuple(dev, in_size, bits_of(in0), bits_of(in1), out_size);
    auto it = cache.find(key);
    if (it != cache.end()) {
        *out = &it->second;
        return IIV_OK;
    }
    // first use of this geometry on this device: made on the host and uploaded synchronously
    Table t;
    t.ksize = ksize_of(in0, in1, out_size);
    const size_t nk = (size_t)out_size * t.ksize;
    std::vector<int32_t> b(2 * (size_t)out_size), k(nk), kt(nk);
    make_coeffs(in_size, in0, in1, out_size, t.ksize, b.data(), k.data());
    t.lo = in_size;
    for (int o = 0; o < out_size; o++) {
        for (int j = 0; j < t.ksize; j++) kt[(size_t)j * out_size + o] = k[(size_t)o * t.ksize + j];
        if (b[2 * o] < t.lo) t.lo = b[2 * o];
        if (b[2 * o] + b[2 * o + 1] > t.hi) t.hi = b[2 * o] + b[2 * o + 1];
    }
    DeviceBuf<int32_t> mem;   // bounds | coefficients by row | by tap
    if (int rc = mem.alloc(b.size() + 2 * nk, "hipMalloc(resize coefficients)")) return rc;
    t.bounds = (int2 *)mem.get();
    t.k_rows = mem + b.size();
    t.k_taps = t.k_rows + nk;
    int rc = hip_check(hipMemcpy(t.bounds, b.data(), b.size() * 4, hipMemcpyHostToDevice), "hipMemcpy(resize bounds)");
    if (!rc) rc = hip_check(hipMemcpy(t.k_rows, k.data(), nk * 4, hipMemcpyHostToDevice), "hipMemcpy(resize coefficients)");
    if (!rc) rc = hip_check(hipMemcpy(t.k_taps, kt.data(), nk * 4, hipMemcpyHostToDevice), "hipMemcpy(resize coefficients)");
    if (rc) return rc;
    (void)mem.release();   // (the cache keeps it for the life of the process)
    *out = &(cache[key] = t);
    return IIV_OK;
}

__device__ inline uint32_t clamp_shift(int32_t acc)
{
    acc >>= kPrecisionBits;
    return (uint32_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

// the dword holding byte p and the next one, shifted so that byte p is byte 0 (p any address; `end` one past the last
// byte that may be read).  Aligned dwords never cross a page, so the first load is safe whenever byte p is.
__device__ inline uint32_t load_unaligned(const uint8_t *p, const uint8_t *end)
{
    const uintptr_t a = (uintptr_t)p & ~(uintptr_t)3;
    const uint32_t s = (uint32_t)((uintptr_t)p & 3);
    const uint32_t d0 = *(const uint32_t *)a;
    const uint32_t d1 = (s && (const uint8_t *)(a + 4) < end) ? *(const uint32_t *)(a + 4) : 0u;
    return __builtin_amdgcn_alignbyte(d1, d0, s);
}

// A row source hands the horizontal pass its pixels.  fill<R>() -- every thread of the workgroup, before its barrier -- unpacks
// rows r0 .. r0 + R - 1 of frame f into px [R][w_pad], a dword r | g << 8 | b << 16 per pixel; from_frame(f0), on the host, is the
// same source f0 frames on; label names the launch in an error.  Two of them: RgbRows here, YuvRows below.
// A source is a WINDOW of its frames (f12): window(c0, r0), on the host, is the same source with column c0 and row r0 as its
// first (multiples of kAlign); rows, w and w_pad are then the window's, and fill() stages nothing outside it.

struct RgbRows {   // packed RGB: rows of 3 w bytes at byte strides, any alignment
    const uint8_t *__restrict__ src;
    size_t fs, rs;
    static constexpr const char *label = "resize_h_kernel<RgbRows> launch";
    static constexpr int kAlign = 1;
    RgbRows from_frame(int f0) const { return {src + (size_t)f0 * fs, fs, rs}; }
    RgbRows window(int c0, int r0) const { return {src + (size_t)r0 * rs + 3 * (size_t)c0, fs, rs}; }

    template <int R>
    __device__ inline void fill(uint32_t *px, unsigned nt, int f, int r0, int rows, int w, int w_pad) const
    {
        const int n4 = w_pad >> 2;
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (r0 + r >= rows) break;
            const uint8_t *row = src + (size_t)f * fs + (size_t)(r0 + r) * rs;
            const uint8_t *end = row + 3 * (size_t)w;
            for (int g = threadIdx.x; g < n4; g += nt) {
                // four pixels = twelve bytes from byte 12 g of the row, in aligned dwords: each one that is read starts inside
                // the row, and an aligned dword never crosses a page, so none can fault
                const uint8_t *p = row + 12 * (size_t)g;
                const uintptr_t a = (uintptr_t)p & ~(uintptr_t)3;
                const uint32_t s = (uint32_t)((uintptr_t)p & 3);
                uint32_t d[4];
#pragma unroll
                for (int j = 0; j < 4; j++) d[j] = (const uint8_t *)(a + 4 * j) < end ? ((const uint32_t *)a)[j] : 0u;
                const uint32_t e0 = __builtin_amdgcn_alignbyte(d[1], d[0], s), e1 = __builtin_amdgcn_alignbyte(d[2], d[1], s),
                               e2 = __builtin_amdgcn_alignbyte(d[3], d[2], s);
                uint4 q;
                q.x = e0 & 0xffffffu;
                q.y = (e0 >> 24) | ((e1 & 0xffffu) << 8);
                q.z = (e1 >> 16) | ((e2 & 0xffu) << 16);
                q.w = e2 >> 8;
                *(uint4 *)&px[r * w_pad + 4 * g] = q;
            }
        }
    }
};

// Horizontal pass: the rows of `src` (rows per frame, w pixels: the window that starts at column c0 of the axis the bounds
// count in) -> dst rows of W pixels (byte strides).  Workgroup = R consecutive rows of one frame; threads = W rounded up to
// waves, one output pixel each.  LDS: R rows of w_pad dwords.
template <int R, class Rows>
__global__ __launch_bounds__(1024) void resize_h_kernel(Rows src, int rows, int w, int c0, int W, const int2 *__restrict__ bounds,
                                                        const int32_t *__restrict__ k_taps, uint8_t *__restrict__ dst,
                                                        size_t dst_fs, size_t dst_rs)
{
    extern __shared__ uint32_t px[];   // [R][w_pad] pixels, r | g << 8 | b << 16
    const int groups = (rows + R - 1) / R;
    const int f = blockIdx.x / groups, r0 = (blockIdx.x % groups) * R;
    const int w_pad = (w + 3) & ~3;
    src.template fill<R>(px, blockDim.x, f, r0, rows, w, w_pad);
    __syncthreads();
    const int x = threadIdx.x;
    if (x >= W) return;
    const int2 bd = bounds[x];
    int32_t acc[R][3];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r][0] = acc[r][1] = acc[r][2] = 1 << (kPrecisionBits - 1);
    const uint32_t *pr = px + (bd.x - c0);
    const int32_t *kp = k_taps + x;
#pragma unroll 4
    for (int j = 0; j < bd.y; j++) {
        const int32_t c = kp[(size_t)j * W];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t v = pr[r * w_pad + j];
            acc[r][0] += __mul24((int)(v & 0xffu), c);
            acc[r][1] += __mul24((int)((v >> 8) & 0xffu), c);
            acc[r][2] += __mul24((int)(v >> 16), c);
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (r0 + r >= rows) break;
        uint8_t *o = dst + (size_t)f * dst_fs + (size_t)(r0 + r) * dst_rs + 3 * (size_t)x;
        o[0] = (uint8_t)clamp_shift(acc[r][0]);
        o[1] = (uint8_t)clamp_shift(acc[r][1]);
        o[2] = (uint8_t)clamp_shift(acc[r][2]);
    }
}

// Vertical pass: src [frames][rows_in][row_bytes] (byte strides; its first row is row `row0` of the axis the bounds count in)
// -> dst [frames][H][row_bytes] (byte strides).  Workgroup = one output row's `blocks_per_row`-th part; thread = four bytes of it.
__global__ __launch_bounds__(256) void resize_v_kernel(const uint8_t *__restrict__ src, size_t src_fs, size_t src_rs, int row0,
                                                       int row_bytes, int H, int blocks_per_row, const int2 *__restrict__ bounds,
                                                       const int32_t *__restrict__ k_rows, int ksize, uint8_t *__restrict__ dst,
                                                       size_t dst_fs, size_t dst_rs)
{
    const int bpr = blocks_per_row;
    const int fy = blockIdx.x / bpr;
    const int f = fy / H, y = fy % H;
    const int j = ((blockIdx.x % bpr) * 256 + threadIdx.x) * 4;
    if (j >= row_bytes) return;
    const int2 bd = bounds[y];
    const int32_t *k = k_rows + (size_t)y * ksize;
    const uint8_t *col = src + (size_t)f * src_fs + (size_t)(bd.x - row0) * src_rs + j;
    int32_t a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int t = 0; t < bd.y; t++) {
        const uint8_t *p = col + (size_t)t * src_rs;
        const uint32_t v = load_unaligned(p, p - j + row_bytes);
        const int32_t c = k[t];
        a0 += __mul24((int)(v & 0xffu), c);
        a1 += __mul24((int)((v >> 8) & 0xffu), c);
        a2 += __mul24((int)((v >> 16) & 0xffu), c);
        a3 += __mul24((int)(v >> 24), c);
    }
    const uint32_t out = clamp_shift(a0) | (clamp_shift(a1) << 8) | (clamp_shift(a2) << 16) | (clamp_shift(a3) << 24);
    uint8_t *o = dst + (size_t)f * dst_fs + (size_t)y * dst_rs + j;
    if (j + 4 <= row_bytes && ((uintptr_t)o & 3) == 0) {
        *(uint32_t *)o = out;
    } else {
        const int nb = row_bytes - j < 4 ? row_bytes - j : 4;
        for (int b = 0; b < nb; b++) o[b] = (uint8_t)(out >> (8 * b));
    }
}

// One launch holds at most 2^32 - 1 work-items in x (and 2^31 - 1 workgroups): frames beyond that go in further launches.
// (1x1 -> 1024x1 is 1024 workgroups of 256 a frame: 16383 frames a launch.)
int frames_per_launch(size_t blocks_per_frame, size_t threads)
{
    const size_t by_items = 0xffffffffu / (blocks_per_frame * threads), by_blocks = 0x7fffffffu / blocks_per_frame;
    const size_t f = by_items < by_blocks ? by_items : by_blocks;
    return f < 1 ? 1 : (f > 0x7fffffff ? 0x7fffffff : (int)f);
}

template <class Rows>
int launch_h(const Rows &src, int frames, int rows, int w, int c0, int W, const Table &t, uint8_t *dst, size_t dst_fs, size_t dst_rs,
             hipStream_t st)
{
    const int threads = (W + 63) & ~63;
    const int w_pad = (w + 3) & ~3;
    const int R = w_pad <= 4096 ? 2 : 1;
    const unsigned bpf = (unsigned)((rows + R - 1) / R);
    const int step = frames_per_launch(bpf, (size_t)threads);
    for (int f0 = 0; f0 < frames; f0 += step) {
        const int fn = frames - f0 < step ? frames - f0 : step;
        if (int rc = launch(R == 2 ? resize_h_kernel<2, Rows> : resize_h_kernel<1, Rows>, Rows::label, dim3((unsigned)fn * bpf), dim3(threads),
                            (size_t)R * w_pad * 4, st, src.from_frame(f0), rows, w, c0, W, t.bounds, t.k_taps, dst + (size_t)f0 * dst_fs,
                            dst_fs, dst_rs))
            return rc;
    }
    return IIV_OK;
}

// (the vertical pass reads packed RGB rows only: a source's, or the horizontal pass's result)
int launch_v(const RgbRows &src, int frames, int row0, int row_bytes, int H, const Table &t, uint8_t *dst, size_t dst_fs,
             size_t dst_rs, hipStream_t st)
{
    const int bpr = (row_bytes + 1023) / 1024;
    const unsigned bpf = (unsigned)H * (unsigned)bpr;
    const int step = frames_per_launch(bpf, 256);
    for (int f0 = 0; f0 < frames; f0 += step) {
        const int fn = frames - f0 < step ? frames - f0 : step;
        if (int rc = launch(resize_v_kernel, "resize_v_kernel launch", dim3((unsigned)fn * bpf), dim3(256), 0, st, src.from_frame(f0).src,
                            src.fs, src.rs, row0, row_bytes, H, bpr, t.bounds, t.k_rows, t.ksize, dst + (size_t)f0 * dst_fs, dst_fs, dst_rs))
            return rc;
    }
    return IIV_OK;
}

// f12: the fill colour over every pixel of dst [frames][H][W][3] outside the rectangle (rx, ry, rw, rh); thread = one pixel.
// The passes write inside the rectangle only, so the fill and they touch no common byte and need no order between them.
__global__ __launch_bounds__(256) void resize_fill_kernel(uint8_t *__restrict__ dst, int H, int W, int rx, int ry, int rw, int rh,
                                                          uint32_t fill, int blocks_per_frame)
{
    const int f = blockIdx.x / blocks_per_frame;
    const int i = (blockIdx.x % blocks_per_frame) * 256 + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    if (y >= ry && y < ry + rh && x >= rx && x < rx + rw) return;
    uint8_t *o = dst + ((size_t)f * H * W + (size_t)i) * 3;
    o[0] = (uint8_t)fill;
    o[1] = (uint8_t)(fill >> 8);
    o[2] = (uint8_t)(fill >> 16);
}

// ---- f11: YUV 4:2:0 sources (include/iivision.h: iiv_resize_frames_yuv420) ------------------------------------
// The conversion is fused into the horizontal pass: YuvRows is resize_h_kernel's second row source.  Where the horizontal pass
// does not come first (same size, vertical only, h > 100 w) yuv_to_rgb_kernel writes the RGB frames of a chunk into a
// stream-ordered scratch and the RGB path takes them from there.

struct YuvMatrix {   // (y_off, ky, rv, gu, gv, bu) of the header, by value in the kernel's arguments
    int32_t y_off, ky, rv, gu, gv, bu;
};

struct YuvSrc {   // the planes of a batch of frames: byte strides, ps = the chroma pixel stride (1 planar, 2 interleaved)
    const uint8_t *y;
    size_t y_fs, y_rs;
    const uint8_t *u, *v;
    size_t c_fs, c_rs;
    int ps;
    YuvSrc from_frame(int f0) const { return {y + (size_t)f0 * y_fs, y_fs, y_rs, u + (size_t)f0 * c_fs, v + (size_t)f0 * c_fs, c_fs, c_rs, ps}; }
};

// what two neighbouring chroma samples add to R, G and B of the pixels under them, the rounding 128 included
struct ChromaTerms {
    int32_t r[2], g[2], b[2];
};

// uu / vv: sample 0 in byte 0, sample 1 in byte ps
__device__ inline ChromaTerms chroma_terms(uint32_t uu, uint32_t vv, int ps, const YuvMatrix &m)
{
    ChromaTerms t;
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int d = (int)((uu >> (8 * ps * s)) & 0xffu) - 128, e = (int)((vv >> (8 * ps * s)) & 0xffu) - 128;
        t.r[s] = __mul24(m.rv, e) + 128;
        t.g[s] = __mul24(m.gu, d) + __mul24(m.gv, e) + 128;
        t.b[s] = __mul24(m.bu, d) + 128;
    }
    return t;
}

// (the empty asm keeps the byte a 32-bit value of its own: where two of them meet as clamp(a >> 8) | clamp(b >> 8) << 8, hipcc
//  selects gfx950's v_ashr_pk_u8_i32 for the pair, and yuv_to_rgb_kernel then stored bytes 2 and 3 of its dwords with bits of
//  the unclamped sums in them on an MI355X -- DESIGN.md 23)
__device__ inline uint32_t clamp_shift8(int32_t v)
{
    v >>= 8;
    uint32_t b = (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    asm volatile("" : "+v"(b));
    return b;
}

// four pixels of one row (yy: pixel j in byte j; samples 0, 0, 1, 1 above them) -> r | g << 8 | b << 16 each
__device__ inline uint4 yuv_to_rgb4(uint32_t yy, const ChromaTerms &t, const YuvMatrix &m)
{
    uint32_t q[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int32_t c = __mul24((int)((yy >> (8 * j)) & 0xffu) - m.y_off, m.ky);
        const int s = j >> 1;
        q[j] = clamp_shift8(c + t.r[s]) | (clamp_shift8(c + t.g[s]) << 8) | (clamp_shift8(c + t.b[s]) << 16);
    }
    return make_uint4(q[0], q[1], q[2], q[3]);
}

// the chroma terms of pixels x .. x + 3 (x even) of source row `row` of frame f, w pixels wide (aligned dword loads inside the
// chroma row only)
__device__ inline ChromaTerms load_chroma(const YuvSrc &s, size_t f, int row, int x, int w, const YuvMatrix &m)
{
    const size_t off = f * s.c_fs + (size_t)(row >> 1) * s.c_rs;
    const size_t len = (size_t)(((w + 1) >> 1) - 1) * s.ps + 1, at = (size_t)(x >> 1) * s.ps;
    const uint8_t *ur = s.u + off, *vr = s.v + off;
    return chroma_terms(load_unaligned(ur + at, ur + len), load_unaligned(vr + at, vr + len), s.ps, m);
}

struct YuvRows {   // 4:2:0 planes, each pixel converted as it is unpacked; the matrix by value: the host copy may change at once
    YuvSrc s;
    YuvMatrix m;
    int fw;       // the frame's width: where a Y row and a chroma row end
    int x0, y0;   // the window's first column and row in the frame, both even: chroma is taken at absolute (y >> 1, x >> 1)
    static constexpr const char *label = "resize_h_kernel<YuvRows> launch";
    static constexpr int kAlign = 2;
    YuvRows from_frame(int f0) const { return {s.from_frame(f0), m, fw, x0, y0}; }
    YuvRows window(int c0, int r0) const { return {s, m, fw, x0 + c0, y0 + r0}; }

    // R = 2: rows (2 k, 2 k + 1), which share their chroma row and its terms (an odd h leaves the last row alone)
    template <int R>
    __device__ inline void fill(uint32_t *px, unsigned nt, int f, int r0, int rows, int w, int w_pad) const
    {
        const int n4 = w_pad >> 2;
        for (int g = threadIdx.x; g < n4; g += nt) {
            const int x = x0 + 4 * g;
            const ChromaTerms t = load_chroma(s, (size_t)f, y0 + r0, x, fw, m);
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (r0 + r >= rows) break;
                const uint8_t *row = s.y + (size_t)f * s.y_fs + (size_t)(y0 + r0 + r) * s.y_rs;
                *(uint4 *)&px[r * w_pad + 4 * g] = yuv_to_rgb4(load_unaligned(row + x, row + fw), t, m);
            }
        }
    }
};

// The conversion alone: thread = four pixels of one row -> twelve bytes of dst [frames][rows][dst_rs], dst 4-byte aligned
// and dst_rs = 3 w_pad (the last group's pad pixels land inside the row's stride).  `total` = frames * rows * w_pad / 4.
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(YuvSrc s, YuvMatrix m, int rows, int w, size_t total,
                                                         uint8_t *__restrict__ dst, size_t dst_fs, size_t dst_rs)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int n4 = (w + 3) >> 2;
    const int g = (int)(i % n4);
    const size_t fr = i / n4, f = fr / rows;
    const int y = (int)(fr % rows);
    const ChromaTerms t = load_chroma(s, f, y, 4 * g, w, m);
    const uint8_t *row = s.y + f * s.y_fs + (size_t)y * s.y_rs;
    const uint4 q = yuv_to_rgb4(load_unaligned(row + 4 * (size_t)g, row + w), t, m);
    uint32_t *o = (uint32_t *)(dst + f * dst_fs + (size_t)y * dst_rs + 12 * (size_t)g);
    o[0] = q.x | (q.y << 24);
    o[1] = (q.y >> 8) | (q.z << 16);
    o[2] = (q.z >> 16) | (q.w << 8);
}

// ---- the host side both entry points share ------------------------------------------------------------------------------------

int check_sizes(const char *entry, int n, int h, int w, int H, int W)
{
    if (n < 0 || h < 1 || h > kMaxIn || w < 1 || w > kMaxIn || H < 1 || H > kMaxOut || W < 1 || W > kMaxOut)
        return set_error(IIV_ERR_INVALID, "%s: n >= 0, h, w in 1..%d, H, W in 1..%d (got n %d, %dx%d -> %dx%d)", entry, kMaxIn, kMaxOut, n,
                         h, w, H, W);
    return IIV_OK;
}

// f12: what of a source frame is resized (box = x0, y0, x1, y1 in source pixels, float32 as Pillow holds it) and where in the
// H x W destination it lands (the rectangle rx, ry, rw, rh); the rest of the destination takes the fill colour
struct Fit {
    float x0, y0, x1, y1;
    int H, W;
    int rx, ry, rw, rh;
    uint32_t fill;
    bool whole_dst() const { return rx == 0 && ry == 0 && rw == W && rh == H; }
};

// iiv_resize_frames' own geometry: the whole frame over the whole destination
Fit stretch(int h, int w, int H, int W) { return {0.0f, 0.0f, (float)w, (float)h, H, W, 0, 0, W, H, 0u}; }

int check_fit(const char *entry, int h, int w, const float *box, int H, int W, const int *rect, uint32_t fill, Fit *g)
{
    if (!box || !rect) return set_error(IIV_ERR_INVALID, "%s: box or rect NULL", entry);
    // (written so that a NaN fails)
    if (!(box[0] >= 0.0f && box[0] < box[2] && box[2] <= (float)w && box[1] >= 0.0f && box[1] < box[3] && box[3] <= (float)h))
        return set_error(IIV_ERR_INVALID, "%s: box (%g, %g, %g, %g) needs 0 <= x0 < x1 <= %d and 0 <= y0 < y1 <= %d", entry, box[0],
                         box[1], box[2], box[3], w, h);
    if (rect[0] < 0 || rect[1] < 0 || rect[2] < 1 || rect[3] < 1 || rect[2] > W - rect[0] || rect[3] > H - rect[1])
        return set_error(IIV_ERR_INVALID, "%s: rect (%d, %d, %d, %d) must lie inside the %dx%d destination with rw, rh >= 1", entry,
                         rect[0], rect[1], rect[2], rect[3], W, H);
    if (fill > 0xffffffu) return set_error(IIV_ERR_INVALID, "%s: fill is r | g << 8 | b << 16, got 0x%x", entry, fill);
    *g = {box[0], box[1], box[2], box[3], H, W, rect[0], rect[1], rect[2], rect[3], fill};
    return IIV_OK;
}

// the frames of one piece of a batch: what kChunkMidBytes hold of `frame_bytes` each, at least 1, at most `cap` (0: none) and n
int frames_per_piece(size_t frame_bytes, size_t cap, int n)
{
    size_t c = kChunkMidBytes / frame_bytes;
    if (c < 1) c = 1;
    if (cap && c > cap) c = cap;
    return c > (size_t)n ? n : (int)c;
}

// Stream-ordered scratch for the length of one call: freed behind the work on its stream.  done(rc, ..) frees it and returns the
// work's status rc, or the free's when the work succeeded; a call that leaves earlier frees it without a report.
class StreamScratch {
public:
    explicit StreamScratch(hipStream_t st) : st_(st) {}
    StreamScratch(const StreamScratch &) = delete;
    StreamScratch &operator=(const StreamScratch &) = delete;
    ~StreamScratch() { if (p_) (void)hipFreeAsync(p_, st_); }
    int alloc(size_t bytes, const char *what) { return hip_check(hipMallocAsync((void **)&p_, bytes, st_), what); }
    int done(int rc, const char *what)
    {
        const int rc_free = p_ ? hip_check(hipFreeAsync(p_, st_), what) : IIV_OK;
        p_ = nullptr;
        return rc ? rc : rc_free;
    }
    uint8_t *get() const { return p_; }

private:
    hipStream_t st_;
    uint8_t *p_ = nullptr;
};

// Pillow's order: the horizontal pass first, unless there is none or the frame is more than a hundred times as tall as wide
// An axis gets a pass when its size changes or the box does not span it (f12 rule 4); the frame's own h and w decide the order.
bool needs_pass(int in_size, float in0, float in1, int out_size) { return out_size != in_size || in0 != 0.0f || in1 != (float)in_size; }
bool horizontal_first(int h, int w, const Fit &g)
{
    return needs_pass(w, g.x0, g.x1, g.rw) && !(needs_pass(h, g.y0, g.y1, g.rh) && h > 100 * w);
}

int launch_fill(int frames, const Fit &g, uint8_t *d_dst, hipStream_t st)
{
    const unsigned bpf = (unsigned)((g.H * g.W + 255) / 256);
    const int step = frames_per_launch(bpf, 256);
    for (int f0 = 0; f0 < frames; f0 += step) {
        const int fn = frames - f0 < step ? frames - f0 : step;
        if (int rc = launch(resize_fill_kernel, "resize_fill_kernel launch", dim3((unsigned)fn * bpf), dim3(256), 0, st,
                            d_dst + (size_t)f0 * 3 * g.H * g.W, g.H, g.W, g.rx, g.ry, g.rw, g.rh, g.fill, (int)bpf))
            return rc;
    }
    return IIV_OK;
}

// n frames of `src` (h, w), the box of g -> the rectangle of g in d_dst (H, W), packed; the fill colour around it.  Only the
// window of the source that the tables touch is staged: columns [c0, c1) of the horizontal table, rows [r0, r1) of the vertical
// one (a source's kAlign rounds c0 and r0 down).  One pass goes straight into the rectangle, in slices of frames that keep the
// grid within range; two go through a stream-ordered scratch, a chunk of frames at a time: (r1 - r0, rw) after a horizontal
// first pass, (rh, c1 - c0) after a vertical one.  The vertical pass reads packed RGB rows only, so it comes first for RgbRows
// alone.
template <class Rows>
int resize_rows(const Rows &src, int n, int h, int w, const Fit &g, uint8_t *d_dst, hipStream_t st)
{
    constexpr bool packed = std::is_same<Rows, RgbRows>::value;
    const bool resize_w = needs_pass(w, g.x0, g.x1, g.rw), resize_h = needs_pass(h, g.y0, g.y1, g.rh), two = resize_w && resize_h;
    const bool h_first = horizontal_first(h, w, g);
    if (!packed && !h_first) return set_error(IIV_ERR_INVALID, "resize_rows: only packed RGB rows can take the vertical pass first");
    const size_t dst_rs = 3 * (size_t)g.W, dst_fs = (size_t)g.H * dst_rs;
    const Table *th = nullptr, *tv = nullptr;
    int rc = IIV_OK;
    // (same size, whole box: Pillow copies; the vertical pass with the in == out table -- one unit tap per row -- is that copy)
    if (resize_w && (rc = get_table(w, g.x0, g.x1, g.rw, &th))) return rc;
    if ((resize_h || !resize_w) && (rc = get_table(h, g.y0, g.y1, g.rh, &tv))) return rc;
    if (!g.whole_dst() && (rc = launch_fill(n, g, d_dst, st))) return rc;
    constexpr int align = ~(Rows::kAlign - 1);
    const int c0 = th ? th->lo & align : 0, c1 = th ? th->hi : w, r0 = tv ? tv->lo & align : 0, r1 = tv ? tv->hi : h;
    const int wc = c1 - c0, hr = r1 - r0;
    const size_t mid_rs = (3 * (size_t)(h_first ? g.rw : wc) + 3) & ~(size_t)3, mid_fs = (size_t)(h_first ? hr : g.rh) * mid_rs;
    const int piece = two ? frames_per_piece(mid_fs, 65536, n) : 65536;
    StreamScratch mid(st);
    if (two && (rc = mid.alloc((size_t)piece * mid_fs, "hipMallocAsync(resize scratch)"))) return rc;
    const RgbRows mid_rows = {mid.get(), mid_fs, mid_rs};
    const size_t fs1 = two ? mid_fs : dst_fs, rs1 = two ? mid_rs : dst_rs;   // where the first pass writes
    for (int f0 = 0; f0 < n && !rc; f0 += piece) {
        const int fn = n - f0 < piece ? n - f0 : piece;
        const Rows s = src.from_frame(f0).window(c0, r0);
        uint8_t *d = d_dst + (size_t)f0 * dst_fs + (size_t)g.ry * dst_rs + 3 * (size_t)g.rx, *d1 = two ? mid.get() : d;
        if (h_first) {
            rc = launch_h(s, fn, hr, wc, c0, g.rw, *th, d1, fs1, rs1, st);
            if (two && !rc) rc = launch_v(mid_rows, fn, r0, 3 * g.rw, g.rh, *tv, d, dst_fs, dst_rs, st);
        } else if constexpr (packed) {
            rc = launch_v(s, fn, r0, 3 * wc, g.rh, *tv, d1, fs1, rs1, st);
            if (two && !rc) rc = launch_h(mid_rows, fn, g.rh, wc, c0, g.rw, *th, d, dst_fs, dst_rs, st);
        }
    }
    return mid.done(rc, "hipFreeAsync(resize scratch)");
}

}  // namespace
}  // namespace iiv

using namespace iiv;

// what iiv_resize_coeffs and iiv_resize_coeffs_box share: the table of the box [in0, in1) of an axis
static int resize_coeffs(const char *entry, int in_size, float in0, float in1, int out_size, int *ksize, int32_t *bounds, int32_t *coeffs)
{
    if (in_size < 1 || in_size > kMaxIn || out_size < 1 || out_size > kMaxOut || !ksize)
        return set_error(IIV_ERR_INVALID, "%s: in_size 1..%d, out_size 1..%d, ksize not NULL (got %d, %d)", entry, kMaxIn, kMaxOut,
                         in_size, out_size);
    if (!(in0 >= 0.0f && in0 < in1 && in1 <= (float)in_size))
        return set_error(IIV_ERR_INVALID, "%s: 0 <= in0 < in1 <= in_size (got %g, %g, %d)", entry, in0, in1, in_size);
    *ksize = ksize_of(in0, in1, out_size);
    if (!bounds && !coeffs) return IIV_OK;
    if (!bounds || !coeffs) return set_error(IIV_ERR_INVALID, "%s: bounds and coeffs both or neither NULL", entry);
    make_coeffs(in_size, in0, in1, out_size, *ksize, bounds, coeffs);
    return IIV_OK;
}

extern "C" int iiv_resize_coeffs(int in_size, int out_size, int *ksize, int32_t *bounds, int32_t *coeffs)
{
    return resize_coeffs("iiv_resize_coeffs", in_size, 0.0f, (float)in_size, out_size, ksize, bounds, coeffs);
}

extern "C" int iiv_resize_coeffs_box(int in_size, const float in_box[2], int out_size, int *ksize, int32_t *bounds, int32_t *coeffs)
{
    if (!in_box) return set_error(IIV_ERR_INVALID, "iiv_resize_coeffs_box: in_box NULL");
    return resize_coeffs("iiv_resize_coeffs_box", in_size, in_box[0], in_box[1], out_size, ksize, bounds, coeffs);
}

// the packed RGB entry points: `entry` names the one that was called in an error, `box` == NULL is the whole frame over the
// whole destination
static int resize_frames_rgb(const char *entry, int n, int h, int w, const uint8_t *d_src, size_t frame_stride, size_t row_stride,
                             const float *box, int H, int W, const int *rect, uint32_t fill, uint8_t *d_dst, void *stream)
{
    if (int rc = check_sizes(entry, n, h, w, H, W)) return rc;
    Fit g = stretch(h, w, H, W);
    if (box || rect)
        if (int rc = check_fit(entry, h, w, box, H, W, rect, fill, &g)) return rc;
    if (n == 0) return IIV_OK;
    const size_t src_row = 3 * (size_t)w, src_frame = (size_t)(h - 1) * row_stride + src_row;
    if (!d_src || !d_dst || row_stride < (h > 1 ? src_row : 0) || (n > 1 && frame_stride < src_frame))
        return set_error(IIV_ERR_INVALID, "%s: d_src / d_dst NULL, or rows / frames overlap (row_stride %zu < %zu or "
                         "frame_stride %zu < %zu)", entry, row_stride, src_row, frame_stride, src_frame);
    return resize_rows(RgbRows{d_src, frame_stride, row_stride}, n, h, w, g, d_dst, (hipStream_t)stream);
}

extern "C" int iiv_resize_frames(int n, int h, int w, const uint8_t *d_src, size_t frame_stride, size_t row_stride, int H, int W,
                                 uint8_t *d_dst, void *stream)
{
    return resize_frames_rgb("iiv_resize_frames", n, h, w, d_src, frame_stride, row_stride, nullptr, H, W, nullptr, 0u, d_dst, stream);
}

extern "C" int iiv_resize_frames_fit(int n, int h, int w, const uint8_t *d_src, size_t frame_stride, size_t row_stride,
                                     const float box[4], int H, int W, const int rect[4], uint32_t fill, uint8_t *d_dst, void *stream)
{
    if (!box || !rect) return set_error(IIV_ERR_INVALID, "iiv_resize_frames_fit: box or rect NULL");
    return resize_frames_rgb("iiv_resize_frames_fit", n, h, w, d_src, frame_stride, row_stride, box, H, W, rect, fill, d_dst, stream);
}

static int resize_frames_yuv(const char *entry, int n, int h, int w, const uint8_t *d_y, size_t y_frame_stride, size_t y_row_stride,
                             const uint8_t *d_u, const uint8_t *d_v, size_t c_frame_stride, size_t c_row_stride, int c_pixel_stride,
                             const int32_t *matrix, const float *box, int H, int W, const int *rect, uint32_t fill, uint8_t *d_dst,
                             void *stream)
{
    if (int rc = check_sizes(entry, n, h, w, H, W)) return rc;
    if (c_pixel_stride != 1 && c_pixel_stride != 2)
        return set_error(IIV_ERR_INVALID, "%s: c_pixel_stride 1 (planar) or 2 (interleaved), got %d", entry, c_pixel_stride);
    if (!matrix) return set_error(IIV_ERR_INVALID, "%s: matrix NULL", entry);
    if (matrix[0] < 0 || matrix[0] > 255) return set_error(IIV_ERR_INVALID, "%s: y_off 0..255, got %d", entry, (int)matrix[0]);
    for (int i = 1; i < 6; i++)
        if (matrix[i] < -1023 || matrix[i] > 1023)
            return set_error(IIV_ERR_INVALID, "%s: coefficients in -1023..1023, matrix[%d] is %d", entry, i, (int)matrix[i]);
    Fit g = stretch(h, w, H, W);
    if (box || rect)
        if (int rc = check_fit(entry, h, w, box, H, W, rect, fill, &g)) return rc;
    if (n == 0) return IIV_OK;
    const int ch = (h + 1) / 2, cw = (w + 1) / 2;
    const size_t y_frame = (size_t)(h - 1) * y_row_stride + (size_t)w;
    const size_t c_row = (size_t)(cw - 1) * c_pixel_stride + 1, c_frame = (size_t)(ch - 1) * c_row_stride + c_row;
    if (!d_y || !d_u || !d_v || !d_dst || (h > 1 && y_row_stride < (size_t)w) || (n > 1 && y_frame_stride < y_frame))
        return set_error(IIV_ERR_INVALID, "%s: a plane or d_dst NULL, or Y rows / frames overlap (y_row_stride %zu < %d "
                         "or y_frame_stride %zu < %zu)", entry, y_row_stride, w, y_frame_stride, y_frame);
    if ((ch > 1 && c_row_stride < c_row) || (n > 1 && c_frame_stride < c_frame))
        return set_error(IIV_ERR_INVALID, "%s: chroma rows / frames overlap (c_row_stride %zu < %zu or c_frame_stride "
                         "%zu < %zu)", entry, c_row_stride, c_row, c_frame_stride, c_frame);
    const hipStream_t st = (hipStream_t)stream;
    const YuvRows src = {{d_y, y_frame_stride, y_row_stride, d_u, d_v, c_frame_stride, c_row_stride, c_pixel_stride},
                         {matrix[0], matrix[1], matrix[2], matrix[3], matrix[4], matrix[5]}, w, 0, 0};
    if (horizontal_first(h, w, g)) return resize_rows(src, n, h, w, g, d_dst, st);
    // the horizontal pass is not the first: convert a chunk of whole frames into scratch (the box's float32 arithmetic counts
    // from the frame's own origin), then the RGB path as it is
    const size_t rgb_rs = 3 * (size_t)((w + 3) & ~3), rgb_fs = (size_t)h * rgb_rs, n4 = (size_t)((w + 3) >> 2);
    const int piece = frames_per_piece(rgb_fs, 0, n);
    StreamScratch rgb(st);
    int rc = rgb.alloc((size_t)piece * rgb_fs, "hipMallocAsync(yuv scratch)");
    if (rc) return rc;
    for (int f0 = 0; f0 < n && !rc; f0 += piece) {
        const int fn = n - f0 < piece ? n - f0 : piece;
        const size_t total = (size_t)fn * h * n4;   // (at most 32 MiB / 12, or one frame's 2^24)
        rc = launch(yuv_to_rgb_kernel, "yuv_to_rgb_kernel launch", dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                    src.s.from_frame(f0), src.m, h, w, total, rgb.get(), rgb_fs, rgb_rs);
        if (!rc) rc = resize_rows(RgbRows{rgb.get(), rgb_fs, rgb_rs}, fn, h, w, g, d_dst + (size_t)f0 * 3 * H * W, st);
    }
    return rgb.done(rc, "hipFreeAsync(yuv scratch)");
}

extern "C" int iiv_resize_frames_yuv420(int n, int h, int w, const uint8_t *d_y, size_t y_frame_stride, size_t y_row_stride,
                                        const uint8_t *d_u, const uint8_t *d_v, size_t c_frame_stride, size_t c_row_stride,
                                        int c_pixel_stride, const int32_t matrix[6], int H, int W, uint8_t *d_dst, void *stream)
{
    return resize_frames_yuv("iiv_resize_frames_yuv420", n, h, w, d_y, y_frame_stride, y_row_stride, d_u, d_v, c_frame_stride,
                             c_row_stride, c_pixel_stride, matrix, nullptr, H, W, nullptr, 0u, d_dst, stream);
}

extern "C" int iiv_resize_frames_yuv420_fit(int n, int h, int w, const uint8_t *d_y, size_t y_frame_stride, size_t y_row_stride,
                                            const uint8_t *d_u, const uint8_t *d_v, size_t c_frame_stride, size_t c_row_stride,
                                            int c_pixel_stride, const int32_t matrix[6], const float box[4], int H, int W,
                                            const int rect[4], uint32_t fill, uint8_t *d_dst, void *stream)
{
    if (!box || !rect) return set_error(IIV_ERR_INVALID, "iiv_resize_frames_yuv420_fit: box or rect NULL");
    return resize_frames_yuv("iiv_resize_frames_yuv420_fit", n, h, w, d_y, y_frame_stride, y_row_stride, d_u, d_v, c_frame_stride,
                             c_row_stride, c_pixel_stride, matrix, box, H, W, rect, fill, d_dst, stream);
}

