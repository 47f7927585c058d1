// iiv_filter.hip -- the spatial filter (f16; include/iivision.h: iiv_filter_frames): per frame a separable 5 x 5 blur B of the
// source p, and per pixel y = p + gain[m] (p - B) with m the largest channel difference -- denoise where the gain is negative,
// unsharp mask where it is positive.  The reference has nothing spatial: its frames reach bmp2dhr as the decoder delivers them.
//
// Shape.  A work item is (clip, frame, tile); a tile is kFilterTileH rows of kFilterTileW pixels, cut at the frame's edges, and a
// workgroup walks the items with a grid stride under iiv_clip.h's cap.  A tile's unit of work is a quad: four pixels of one row,
// three dwords, iiv_clip.h's lane; the quads of a tile are numbered row by row over the tile's own width (q = row * qw + column)
// and dealt to the lanes in turn, so a narrow frame (280 wide: 70 quads a row) leaves no lane idle but in the last round.
//   * Horizontal pass: for every quad of the tile's rows and of kFilterHalo rows above and below (row indices clamped to the
//     frame: the replicated edge), a lane loads the quad's three dwords and the two dwords on either side (two pixels each; at the
//     frame's left and right edge the edge pixel instead), and writes the twelve h values to LDS as u16 -- at most 256 * 255 =
//     65280, exact.  The LDS index of a quad is its number q: rows are dense over the tile's own width.
//   * Vertical pass: the quad under halo row r + j is q + j * qw; five reads of twelve u16, B = (sum + 32768) >> 16 (at most
//     256 * 65280 + 32768 < 2^24), the source quad once more from memory (it is in cache: this workgroup has just read it), m, the
//     gain from LDS, the blend, one dwordx3 store.
//   * gain[256] and the ten taps come by value; the gain is staged in LDS once per workgroup, the taps are wave-uniform.
// Every source byte is read once from memory plus the halo rows ((T_h + 4) / T_h) and the side dwords, which the cache serves.
// Nothing is allocated, nothing synchronised, nothing kept between calls.
#include "iiv_clip.h"
#include "iiv_host.h"

namespace iiv {

namespace {

constexpr int kFilterTileH = 16;            // rows of a tile
constexpr int kFilterTileW = 320;           // pixels of a tile's row: 80 quads
constexpr int kFilterHalo = 2;              // rows above and below, pixels left and right: a 5-tap axis
constexpr int kFilterQuadsW = kFilterTileW / kClipLanePixels;
constexpr int kFilterRows = kFilterTileH + 2 * kFilterHalo;

struct FilterParams {
    uint16_t taps_x[5], taps_y[5];
    int16_t gain[256];
};

// the twelve h values of a quad, two to a dword: value i is the low (i even) or high half of v[i / 2]
struct alignas(8) Quad16 { uint32_t v[6]; };
__device__ static inline uint32_t quad16_get(const Quad16 &a, int i) { return (a.v[i >> 1] >> (16 * (i & 1))) & 0xffffu; }

__global__ __launch_bounds__(kClipThreads) void filter_kernel(size_t n_items, int n_frames, int height, int width, int tiles_y, int tiles_x,
                                                              const uint8_t *src, size_t src_clip_stride, size_t src_frame_stride,
                                                              uint8_t *out, size_t out_clip_stride, size_t out_frame_stride,
                                                              const FilterParams P)
{
    __shared__ Quad16 h_s[kFilterRows * kFilterQuadsW];
    __shared__ int16_t gain_s[256];
    const int tid = threadIdx.x;
    gain_s[tid] = P.gain[tid];   // (kClipThreads == 256; the first barrier below is in front of its first reader)
    const size_t row_bytes = (size_t)width * 3;
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        size_t rest = item;
        const int tile_x = (int)(rest % (size_t)tiles_x);
        rest /= (size_t)tiles_x;
        const int tile_y = (int)(rest % (size_t)tiles_y);
        rest /= (size_t)tiles_y;
        const size_t frame = rest % (size_t)n_frames, clip = rest / (size_t)n_frames;
        const int x0 = tile_x * kFilterTileW, y0 = tile_y * kFilterTileH;
        const int qw = (width - x0 < kFilterTileW ? width - x0 : kFilterTileW) / kClipLanePixels;   // quads of this tile's rows
        const int th = height - y0 < kFilterTileH ? height - y0 : kFilterTileH;                     // rows of this tile
        const uint8_t *s = src + clip * src_clip_stride + frame * src_frame_stride;
        uint8_t *o = out + clip * out_clip_stride + frame * out_frame_stride;

        // ---- horizontal: halo row r of the tile is source row clamp(y0 + r - kFilterHalo)
        for (int q = tid; q < (th + 2 * kFilterHalo) * qw; q += kClipThreads) {
            const int r = q / qw, c = q - r * qw;
            int sy = y0 + r - kFilterHalo;
            sy = sy < 0 ? 0 : sy > height - 1 ? height - 1 : sy;
            const int x = x0 + c * kClipLanePixels;
            const uint8_t *at = s + (size_t)sy * row_bytes + (size_t)x * 3;
            const Dwords3 a = *reinterpret_cast<const Dwords3 *>(at);
            // p[c][i]: channel c of pixel x - 2 + i, i = 0..7
            uint32_t p[3][8];
#pragma unroll
            for (int i = 0; i < kClipLanePixels; i++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) p[ch][kFilterHalo + i] = clip_byte(a, 3 * i + ch);
            if (x > 0) {   // bytes -8..-1: pixels x - 2 and x - 1 are bytes -6..-1
                const uint32_t l0 = *reinterpret_cast<const uint32_t *>(at - 8), l1 = *reinterpret_cast<const uint32_t *>(at - 4);
                p[0][0] = l0 >> 16 & 0xffu, p[1][0] = l0 >> 24, p[2][0] = l1 & 0xffu;
                p[0][1] = l1 >> 8 & 0xffu, p[1][1] = l1 >> 16 & 0xffu, p[2][1] = l1 >> 24;
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ch++) p[ch][0] = p[ch][1] = p[ch][kFilterHalo];
            }
            if (x + kClipLanePixels < width) {   // bytes 12..19: pixels x + 4 and x + 5 are bytes 12..17
                const uint32_t r0 = *reinterpret_cast<const uint32_t *>(at + 12), r1 = *reinterpret_cast<const uint32_t *>(at + 16);
                p[0][6] = r0 & 0xffu, p[1][6] = r0 >> 8 & 0xffu, p[2][6] = r0 >> 16 & 0xffu;
                p[0][7] = r0 >> 24, p[1][7] = r1 & 0xffu, p[2][7] = r1 >> 8 & 0xffu;
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ch++) p[ch][6] = p[ch][7] = p[ch][kFilterHalo + kClipLanePixels - 1];
            }
            uint32_t h[kClipLanePixels * 3];
#pragma unroll
            for (int i = 0; i < kClipLanePixels; i++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    uint32_t acc = 0;
#pragma unroll
                    for (int k = 0; k < 5; k++) acc += (uint32_t)P.taps_x[k] * p[ch][i + k];
                    h[3 * i + ch] = acc;
                }
            Quad16 hq;
#pragma unroll
            for (int i = 0; i < 6; i++) hq.v[i] = h[2 * i] | h[2 * i + 1] << 16;
            h_s[q] = hq;
        }
        __syncthreads();

        // ---- vertical, gain and blend: output row r of the tile has its five h rows at halo rows r..r + 4
        for (int q = tid; q < th * qw; q += kClipThreads) {
            const int r = q / qw, c = q - r * qw;
            const size_t at = (size_t)(y0 + r) * row_bytes + (size_t)(x0 + c * kClipLanePixels) * 3;
            const Dwords3 a = *reinterpret_cast<const Dwords3 *>(s + at);
            uint32_t acc[kClipLanePixels * 3];
#pragma unroll
            for (int i = 0; i < kClipLanePixels * 3; i++) acc[i] = 32768u;
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const Quad16 hq = h_s[q + j * qw];
#pragma unroll
                for (int i = 0; i < kClipLanePixels * 3; i++) acc[i] += (uint32_t)P.taps_y[j] * quad16_get(hq, i);
            }
            uint32_t y[kClipLanePixels * 3];
#pragma unroll
            for (int i = 0; i < kClipLanePixels; i++) {
                int pc[3], d[3], m = 0;
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    pc[ch] = (int)clip_byte(a, 3 * i + ch);
                    d[ch] = pc[ch] - (int)(acc[3 * i + ch] >> 16);
                    const int ad = d[ch] < 0 ? -d[ch] : d[ch];
                    m = ad > m ? ad : m;
                }
                const int g = gain_s[m];
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const int v = pc[ch] + ((g * d[ch] + 128) >> 8);   // (an arithmetic shift: floor towards minus infinity)
                    y[3 * i + ch] = (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
                }
            }
            Dwords3 yq;
#pragma unroll
            for (int i = 0; i < 3; i++) yq.v[i] = clip_pack4(y[4 * i], y[4 * i + 1], y[4 * i + 2], y[4 * i + 3]);
            *reinterpret_cast<Dwords3 *>(o + at) = yq;
        }
        __syncthreads();   // (the next item's horizontal pass overwrites h_s)
    }
}

}  // namespace

}  // namespace iiv

using namespace iiv;

extern "C" {

int iiv_filter_frames(int n_clips, int n_frames, int height, int width, const uint8_t *d_src, size_t src_clip_stride,
                      size_t src_frame_stride, uint8_t *d_out, size_t out_clip_stride, size_t out_frame_stride,
                      const uint16_t taps_x[5], const uint16_t taps_y[5], const int16_t gain[256], void *stream)
{
    if (int rc = clip_refuse("iiv_filter_frames", n_clips, n_frames, (long)height * (long)width, 24,
                             (uintptr_t)d_src | (uintptr_t)d_out | src_clip_stride | src_frame_stride | out_clip_stride | out_frame_stride,
                             {src_frame_stride, out_frame_stride}))
        return rc;
    if (height < 1 || height > 4096) return set_error(IIV_ERR_INVALID, "iiv_filter_frames: height must be 1..4096, got %d", height);
    if (width < 4 || width > 4096 || width % kClipLanePixels)
        return set_error(IIV_ERR_INVALID, "iiv_filter_frames: width must be a multiple of 4 in 4..4096, got %d", width);
    if (!taps_x || !taps_y || !gain) return set_error(IIV_ERR_INVALID, "iiv_filter_frames: NULL taps or gain");
    FilterParams P;
    for (int axis = 0; axis < 2; axis++) {
        const uint16_t *taps = axis ? taps_y : taps_x;
        unsigned sum = 0;
        for (int k = 0; k < 5; k++) {
            if (taps[k] > 256) return set_error(IIV_ERR_INVALID, "iiv_filter_frames: a tap above 256 (%u)", (unsigned)taps[k]);
            sum += taps[k];
            (axis ? P.taps_y : P.taps_x)[k] = taps[k];
        }
        if (sum != 256) return set_error(IIV_ERR_INVALID, "iiv_filter_frames: the taps of an axis must sum to 256, got %u", sum);
    }
    for (int m = 0; m < 256; m++) {
        if (gain[m] < -256 || gain[m] > 1024)
            return set_error(IIV_ERR_INVALID, "iiv_filter_frames: gain[%d] = %d is outside -256..1024", m, (int)gain[m]);
        P.gain[m] = gain[m];
    }
    if (d_src && d_out == d_src) return set_error(IIV_ERR_INVALID, "iiv_filter_frames: d_out == d_src (a neighbour's source would be overwritten)");
    if (n_clips == 0 || n_frames == 0) return IIV_OK;
    if (!d_src || !d_out) return set_error(IIV_ERR_INVALID, "iiv_filter_frames: a NULL pointer");
    const int tiles_y = (height + kFilterTileH - 1) / kFilterTileH, tiles_x = (width + kFilterTileW - 1) / kFilterTileW;
    const size_t n_items = (size_t)n_clips * (size_t)n_frames * (size_t)tiles_y * (size_t)tiles_x;
    return launch(filter_kernel, "filter_kernel launch", dim3(clip_grid(n_items)), dim3(kClipThreads), 0, (hipStream_t)stream, n_items,
                  n_frames, height, width, tiles_y, tiles_x, d_src, src_clip_stride, src_frame_stride, d_out, out_clip_stride,
                  out_frame_stride, P);
}

}  // extern "C"
