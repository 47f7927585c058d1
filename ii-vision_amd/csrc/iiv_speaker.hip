// iiv_speaker.hip -- tick bytes -> the 16-bit PCM the player's speaker toggles make (f13: speaker preview; include/iivision.h:
// iiv_speaker_pcm).  The reference has no such thing: player/main.s toggles the speaker at the start of every 73-cycle opcode
// and `tick` cycles later, and what that sounds like could only be heard on the machine.
//
// Shape.  The kernel only streams: it reads one byte per 73 cycles and writes two per `decim` cycles.
//   * No cycle is ever visited.  H[j] is the sum of the filter's first j taps (at most 290 ints, built on the host, passed by
//     value, copied to LDS once per workgroup).  A sample's window of order * (decim - 1) + 1 cycles touches at most five
//     periods; the pulse of a period covers a run of consecutive taps, whose sum is a difference of two entries of H.  So
//     acc = -decim^order + 2 * (sum of those differences).
//   * The period -> opcode map is the closed form of the header (ACK periods after opcodes 290, 582, ...): no prefix scan.
//   * A workgroup takes a run of kSpeakerRun consecutive samples of one stream.  The widths of the periods the run touches
//     are staged in LDS as bytes, one period a thread, consecutive threads consecutive tick bytes (the legality check and the
//     two off-by-one widths are applied there).  A thread then computes eight consecutive samples and writes them as one
//     16-byte store where the row allows it: consecutive lanes, consecutive addresses, 1 KiB a wave instruction.
//   * The list of (stream, run) items is walked with a grid stride under kSpeakerGridCap workgroups.
// The scaling's floor division by decim^order is a double multiply by the reciprocal, corrected by the 64-bit remainder: exact.
// Nothing is allocated, nothing synchronised.
#include "iiv_host.h"

namespace iiv {

namespace {

constexpr int kSpeakerPeriod = 73;          // cycles of one opcode (player/main.s)
constexpr int kSpeakerAckWidth = 34;        // op_ack and checkrecv toggle at 0 and 34
constexpr int kSpeakerMaxDecim = 73;
constexpr int kSpeakerMaxOrder = 4;
constexpr int kSpeakerTable = kSpeakerMaxOrder * (kSpeakerMaxDecim - 1) + 2;   // entries of H: taps + 1 = 290
constexpr int kSpeakerThreads = 256;
constexpr int kSpeakerPerThread = 8;        // consecutive samples of a thread: one 16-byte store
constexpr int kSpeakerRun = 2048;           // samples of one work item
constexpr int kSpeakerGridCap = 2048;       // workgroups of a launch; the items beyond are reached by the grid stride
constexpr int kSpeakerStage = kSpeakerRun + 8;   // periods a run can touch: (2047 * 73 + 288) / 73 + 2 <= 2054

static_assert(kSpeakerRun == kSpeakerThreads * kSpeakerPerThread, "a thread takes eight samples of its workgroup's run");

struct SpeakerFilter {
    int32_t sum[kSpeakerTable];   // sum[j] = h[0] + ... + h[j - 1]; sum[taps] = decim^order <= 73^4 < 2^25
};

// ACKs in front of opcode k
__host__ __device__ inline long speaker_acks(long k) { return k < 291 ? 0 : 1 + (k - 291) / 292; }

// the width of period p of a stream: its opcode's tick through width(), or an ACK's 34.  bad: the tick byte was illegal
__device__ inline int speaker_width(const uint8_t *__restrict__ ticks, long p, bool *bad)
{
    long k = p;
    if (p >= 291) {
        const long u = p - 291, g = u / 294, r = u - 294 * g;   // after opcode 290: [ACK, ACK, 292 opcodes] repeating
        if (r < 2) return kSpeakerAckWidth;
        k = 291 + 292 * g + (r - 2);
    }
    const int t = ticks[k];
    if ((t & 1) || t < 4 || t > 66) {
        *bad = true;
        return 0;
    }
    return t == 22 ? 21 : (t == 40 ? 41 : t);
}

__global__ __launch_bounds__(kSpeakerThreads) void speaker_kernel(size_t n_items, size_t runs, const uint8_t *__restrict__ ticks,
                                                                  size_t ticks_stride, const int64_t *__restrict__ counts,
                                                                  size_t counts_stride, int decim, int taps, long full,
                                                                  double inv_full, int gain, const SpeakerFilter F,
                                                                  int16_t *__restrict__ pcm, size_t pcm_stride, int *err)
{
    __shared__ int32_t sum_s[kSpeakerTable];
    __shared__ uint8_t width_s[kSpeakerStage];
    const int tid = threadIdx.x;
    for (int i = tid; i < kSpeakerTable; i += kSpeakerThreads) sum_s[i] = F.sum[i];
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t s = item / runs;
        const long m0 = (long)(item - s * runs) * kSpeakerRun;
        long n = counts[s * counts_stride];
        n = n < 0 ? 0 : (n > (long)ticks_stride ? (long)ticks_stride : n);
        const long Q = n + 2 * speaker_acks(n);
        const long M = (kSpeakerPeriod * Q + decim - 1) / decim;
        if (m0 >= M) continue;   // (the same in every thread)
        const int n_run = M - m0 < kSpeakerRun ? (int)(M - m0) : kSpeakerRun;
        // the periods the run's windows touch: [p0, p0 + n_p)
        const long c_first = m0 * decim + decim - taps;                      // the lowest cycle of sample m0's window
        const long p0 = c_first > 0 ? c_first / kSpeakerPeriod : 0;
        const long c_last = (m0 + n_run - 1) * decim + decim - 1;            // the highest cycle of the run's last window
        long p1 = c_last / kSpeakerPeriod;
        p1 = p1 < Q ? p1 : Q - 1;
        int n_p = (int)(p1 - p0 + 1);
        n_p = n_p < kSpeakerStage ? n_p : kSpeakerStage;
        bool bad = false;
        const uint8_t *row = ticks + s * ticks_stride;
        for (int i = tid; i < n_p; i += kSpeakerThreads) width_s[i] = (uint8_t)speaker_width(row, p0 + i, &bad);
        if (bad && err) *err = 1;
        __syncthreads();
        // eight consecutive samples; cycles are counted from the start of period p0 from here on (they fit an int)
        const int j0 = tid * kSpeakerPerThread;
        uint32_t packed[kSpeakerPerThread / 2] = {0, 0, 0, 0};
        if (j0 < n_run) {
            const int hi0 = (int)((m0 + j0) * decim + decim - 1 - p0 * kSpeakerPeriod);
#pragma unroll
            for (int e = 0; e < kSpeakerPerThread; e++) {
                const int hi = hi0 + e * decim, lo = hi - (taps - 1);        // the window [lo, hi]; tap i meets cycle hi - i
                const int pa = (lo > 0 ? lo : 0) / kSpeakerPeriod;
                int pb = hi / kSpeakerPeriod;
                pb = pb < n_p ? pb : n_p - 1;
                int sum = 0;
                for (int p = pa; p <= pb; p++) {
                    const int start = p * kSpeakerPeriod;
                    const int a = start > lo ? start : lo;                   // the pulse's cycles inside the window: [a, b)
                    const int end = start + width_s[p];
                    const int b = end < hi + 1 ? end : hi + 1;
                    if (a < b) sum += sum_s[hi - a + 1] - sum_s[hi - b + 1];
                }
                const long prod = (long)(2 * sum - (int)full) * gain;
                long q = (long)floor((double)prod * inv_full);               // within one of the quotient; the remainder decides
                const long r = prod - q * full;
                q += r < 0 ? -1 : (r >= full ? 1 : 0);
                q = q < -32768 ? -32768 : (q > 32767 ? 32767 : q);
                packed[e >> 1] |= ((uint32_t)q & 0xffffu) << (16 * (e & 1));
            }
            int16_t *dst = pcm + s * pcm_stride + m0 + j0;
            if (j0 + kSpeakerPerThread <= n_run && ((uintptr_t)dst & 15) == 0) {
                *reinterpret_cast<uint4 *>(dst) = make_uint4(packed[0], packed[1], packed[2], packed[3]);
            } else {
                const int k_end = n_run - j0 < kSpeakerPerThread ? n_run - j0 : kSpeakerPerThread;
                for (int e = 0; e < k_end; e++) dst[e] = (int16_t)(packed[e >> 1] >> (16 * (e & 1)));
            }
        }
        __syncthreads();   // (the next item's widths are written behind these reads)
    }
}

}  // namespace

}  // namespace iiv

using namespace iiv;

extern "C" {

long iiv_speaker_periods(long n_ops)
{
    const long n = n_ops < 0 ? 0 : n_ops;
    return n + 2 * speaker_acks(n);
}

long iiv_speaker_sample_count(long n_ops, int decim)
{
    if (decim < 1 || decim > kSpeakerMaxDecim) return set_error(IIV_ERR_INVALID, "speaker_sample_count: decim must be 1..73");
    return (kSpeakerPeriod * iiv_speaker_periods(n_ops) + decim - 1) / decim;
}

int iiv_speaker_pcm(int n_streams, const uint8_t *d_ticks, size_t ticks_stride, const int64_t *d_counts, size_t counts_stride,
                    int decim, int order, int gain, int16_t *d_pcm, size_t pcm_stride, int *d_err, void *stream)
{
    if (decim < 1 || decim > kSpeakerMaxDecim || order < 1 || order > kSpeakerMaxOrder || gain < 0 || gain > 32767)
        return set_error(IIV_ERR_INVALID, "iiv_speaker_pcm: decim 1..73, order 1..4, gain 0..32767");
    if (n_streams < 0 || !d_ticks || !d_counts || !d_pcm)
        return set_error(IIV_ERR_INVALID, "iiv_speaker_pcm: n_streams < 0 or a NULL pointer");
    if (((uintptr_t)d_counts & 7) || ((uintptr_t)d_pcm & 1) || ((uintptr_t)d_err & 3))
        return set_error(IIV_ERR_INVALID, "iiv_speaker_pcm: d_counts must be 8-byte aligned, d_pcm 2-byte, d_err 4-byte");
    if (ticks_stride > (size_t)1 << 48) return set_error(IIV_ERR_INVALID, "iiv_speaker_pcm: ticks_stride above 2^48");
    const long m_max = iiv_speaker_sample_count((long)ticks_stride, decim);
    if (pcm_stride < (size_t)m_max)
        return set_error(IIV_ERR_INVALID, "iiv_speaker_pcm: pcm_stride %zu is below the %ld samples of %zu opcodes", pcm_stride, m_max,
                         ticks_stride);
    const size_t runs = ((size_t)m_max + kSpeakerRun - 1) / kSpeakerRun;
    const size_t n_items = (size_t)n_streams * runs;
    if (n_items == 0) return IIV_OK;
    // the running sum of h_order, h_order built by repeated convolution with `decim` ones
    SpeakerFilter F;
    long h[kSpeakerTable] = {1}, next[kSpeakerTable];
    int taps = 1;
    for (int r = 0; r < order; r++) {
        const int grown = taps + decim - 1;
        for (int i = 0; i < grown; i++) {
            long v = 0;
            for (int j = 0; j < decim; j++)
                if (i - j >= 0 && i - j < taps) v += h[i - j];
            next[i] = v;
        }
        memcpy(h, next, sizeof(long) * grown);
        taps = grown;
    }
    long run = 0;
    for (int j = 0; j < kSpeakerTable; j++) {
        F.sum[j] = (int32_t)run;
        if (j < taps) run += h[j];
    }
    const long full = run;   // decim^order
    const unsigned grid = (unsigned)(n_items < (size_t)kSpeakerGridCap ? n_items : (size_t)kSpeakerGridCap);
    return launch(speaker_kernel, "speaker_kernel launch", dim3(grid), dim3(kSpeakerThreads), 0, (hipStream_t)stream, n_items, runs,
                  d_ticks, ticks_stride, d_counts, counts_stride, decim, taps, full, 1.0 / (double)full, gain, F, d_pcm, pcm_stride,
                  d_err);
}

}  // extern "C"
