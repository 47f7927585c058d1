// iiv_audio.hip -- the audio track: interleaved int16 PCM -> speaker duty-cycle ticks, batched over streams and blocks.
// Reference: audio.Audio._decode / _normalization / audio_stream (transcoder/audio.py:47-107) and the tick of
// movie.Movie.encode (movie.py:104-111).  The reference resamples each decode block with scipy.signal.resample (librosa
// 0.9.2, res_type='scipy', scale=True); the same arithmetic is done here with complex fp32 FFTs:
//   - a radix-2 FFT of 2^a <= 4096 points per transform in LDS, several transforms per workgroup for short ones;
//   - sizes 2^13 .. 2^24 as two such passes through global memory (four-step: columns, twiddle, rows);
//   - every other length (the 43691-point inverse of a 131072-frame block, short last blocks, the normalisation prefix)
//     by Bluestein's chirp-z convolution on the next power of two >= 2L-1, chirp phases from n^2 mod 2L in 64-bit integers.
// Twiddles, chirps and the chirp spectra are computed in fp64 and stored as fp32 (cached per size).
#include "iiv_host.h"

#include <math.h>

#include <map>
#include <utility>
#include <vector>

namespace iiv {

namespace {

constexpr int kFftMaxLog = 12;            // one LDS pass: 2^12 complex fp32 = 32 KiB
constexpr int kFftMaxLogTotal = 24;       // two passes
constexpr long kPrefixBytes = 10L << 20;  // audio.py:63 read_bytes
constexpr long kRawBlockFrames = 1024;    // audioread rawread read_data() default block (assumption A2)

// one decode block of one stream
struct Job {
    long pcm_off;    // int16 element of the block's first sample
    long out_off;    // tick (byte) or float element of the block's first output sample
    int channels;
    float scale;     // 1 / (Nx * sqrt(ratio)) (audio.py:56-58: irfft's 1/num, resample's num/Nx, librosa's scale)
    float norm;      // Audio.normalization (ticks) -- unused for float output
};

__host__ __device__ inline float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// ---- tables ---------------------------------------------------------------------------------------------------------

// tw[j] = exp(-2 pi i j / L), j < L
__global__ __launch_bounds__(256) void twiddle_kernel(float2 *tw, long L)
{
    long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= L) return;
    double s, c;
    sincospi(-2.0 * (double)j / (double)L, &s, &c);
    tw[j] = make_float2((float)c, (float)s);
}

// chirp[n] = exp(dir * i pi n^2 / L), n < L; the phase from n^2 mod 2L (exact in 64 bits for L < 2^31)
__global__ __launch_bounds__(256) void chirp_kernel(float2 *chirp, long L, int dir)
{
    long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= L) return;
    long q = (long)(((unsigned long long)n * (unsigned long long)n) % (unsigned long long)(2 * L));
    double s, c;
    sincospi((double)dir * (double)q / (double)L, &s, &c);
    chirp[n] = make_float2((float)c, (float)s);
}

// b[m] = conj(chirp[|m|]) / M on the circle of M points (m in (-L, L)), zero elsewhere
__global__ __launch_bounds__(256) void bluestein_b_kernel(float2 *b, long L, long M, int dir)
{
    long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    long n = m < L ? m : (m > M - L ? M - m : -1);
    float2 v = make_float2(0.f, 0.f);
    if (n >= 0) {
        long q = (long)(((unsigned long long)n * (unsigned long long)n) % (unsigned long long)(2 * L));
        double s, c;
        sincospi(-(double)dir * (double)q / (double)L, &s, &c);
        v = make_float2((float)(c / (double)M), (float)(s / (double)M));
    }
    b[m] = v;
}

// ---- the FFT --------------------------------------------------------------------------------------------------------

// C transforms of L = 2^logL points per workgroup (C * L <= 4096), unnormalised, sign dir (-1 forward, +1 inverse).
// Transform t reads in[(t / inner) * outer + (t % inner) * in_bs + i * in_es] (i < L), optionally times
// premul[(t % inner) * in_bs + i * in_es], and writes element k to out[(t / inner) * outer + (t % inner) * out_bs + k * out_es],
// optionally times exp(dir 2 pi i ((t % inner) * k mod Ltot) / Ltot) (post_tw: the Ltot-point table; the four-step twiddle).
// Loads and stores walk the transforms fastest when the element stride is not 1, so that neighbouring lanes touch
// neighbouring columns.  in == out is allowed when every transform writes only the addresses it reads.
__global__ __launch_bounds__(256) void fft_lds_kernel(const float2 *in, float2 *out, int logL, int C, long n_t, long inner,
                                                      long outer, long in_bs, long in_es, long out_bs, long out_es,
                                                      const float2 *__restrict__ tw, int dir, const float2 *__restrict__ premul,
                                                      const float2 *__restrict__ post_tw, long tot_mask)
{
    __shared__ float2 s[1 << kFftMaxLog];
    const int L = 1 << logL;
    const int CL = C * L;
    const long t0 = (long)blockIdx.x * C;
    for (int e = threadIdx.x; e < CL; e += 256) {
        int c, i;
        if (in_es == 1) { c = e >> logL; i = e & (L - 1); }
        else { c = e % C; i = e / C; }
        long t = t0 + c;
        float2 v = make_float2(0.f, 0.f);
        if (t < n_t) {
            long off = (t % inner) * in_bs + (long)i * in_es;
            v = in[(t / inner) * outer + off];
            if (premul) v = cmul(v, premul[off]);
        }
        int r = logL ? (int)(__brev((unsigned)i) >> (32 - logL)) : 0;
        s[c * L + r] = v;
    }
    __syncthreads();
    for (int len = 2, lg = 1; len <= L; len <<= 1, lg++) {
        const int half = len >> 1;
        for (int u = threadIdx.x; u < CL / 2; u += 256) {
            int c = u >> (logL - 1), b = u & (L / 2 - 1);
            int j = b & (half - 1);
            int base = c * L + ((b >> (lg - 1)) << lg);
            float2 w = tw[(long)j << (logL - lg)];
            if (dir > 0) w.y = -w.y;
            float2 x0 = s[base + j], x1 = cmul(s[base + j + half], w);
            s[base + j] = make_float2(x0.x + x1.x, x0.y + x1.y);
            s[base + j + half] = make_float2(x0.x - x1.x, x0.y - x1.y);
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < CL; e += 256) {
        int c, k;
        if (out_es == 1) { c = e >> logL; k = e & (L - 1); }
        else { c = e % C; k = e / C; }
        long t = t0 + c;
        if (t >= n_t) continue;
        float2 v = s[c * L + k];
        if (post_tw) {
            float2 w = post_tw[((t % inner) * (long)k) & tot_mask];
            if (dir > 0) w.y = -w.y;
            v = cmul(v, w);
        }
        out[(t / inner) * outer + (t % inner) * out_bs + (long)k * out_es] = v;
    }
}

// Device memory of one call or of one group of blocks: stream-ordered allocations, all freed (stream-ordered, behind the
// work that uses them) when the scope ends -- nothing outlives a call and nothing waits for the device.  The twiddles of a
// call are shared by its groups (at most one table per power of two); the chirp tables of a length live in its group's
// scope, so a batch of many distinct lengths holds one group's tables at a time.
struct Scratch {
    hipStream_t st;
    std::vector<void *> mem;
    std::map<int, float2 *> tw;   // log2 size -> twiddles
    explicit Scratch(hipStream_t s) : st(s) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch()
    {
        for (void *p : mem) (void)hipFreeAsync(p, st);
    }
    template <typename T>
    int alloc(T **p, size_t count, const char *what)
    {
        void *v = nullptr;
        if (int rc = hip_check(hipMallocAsync(&v, sizeof(T) * (count ? count : 1), st), what)) return rc;
        mem.push_back(v);
        *p = (T *)v;
        return IIV_OK;
    }
};

int log2_exact(long L)
{
    int a = 0;
    while ((1L << a) < L) a++;
    return a;
}

// tw[j] = exp(-2 pi i j / 2^a), made once per call and size
int twiddles(Scratch &call, int a, const float2 **out)
{
    auto it = call.tw.find(a);
    if (it != call.tw.end()) {
        *out = it->second;
        return IIV_OK;
    }
    const long L = 1L << a;
    float2 *d = nullptr;
    if (int rc = call.alloc(&d, (size_t)L, "hipMallocAsync(twiddles)")) return rc;
    if (int rc = launch(twiddle_kernel, "twiddle_kernel launch", dim3((unsigned)((L + 255) / 256)), dim3(256), 0, call.st, d, L)) return rc;
    call.tw[a] = d;
    *out = d;
    return IIV_OK;
}

// Ltot = 2^a points for each of n_sig signals laid out contiguously (signal g at g * Ltot): x -> FFT_dir(x) (times premul
// elementwise first, if given).  The result is in *buf or *tmp; *result says which.  a = 0: the identity.
int fft(Scratch &call, float2 *buf, float2 *tmp, int a, long n_sig, int dir, const float2 *premul, float2 **result)
{
    hipStream_t st = call.st;
    const long L = 1L << a;
    if (a == 0) {
        if (premul) return set_error(IIV_ERR_INVALID, "fft: premul of a 1-point transform");
        *result = buf;
        return IIV_OK;
    }
    if (a <= kFftMaxLog) {
        const float2 *tw;
        if (int rc = twiddles(call, a, &tw)) return rc;
        int C = (1 << kFftMaxLog) >> a;
        long n_t = n_sig;
        if (int rc = launch(fft_lds_kernel, "fft_lds_kernel launch", dim3((unsigned)((n_t + C - 1) / C)), dim3(256), 0, st, buf, buf, a, C, n_t,
                            1L, L, 0L, 1L, 0L, 1L, tw, dir, premul, (const float2 *)nullptr, 0L))
            return rc;
        *result = buf;
        return IIV_OK;
    }
    if (a > kFftMaxLogTotal) return set_error(IIV_ERR_INVALID, "fft: 2^%d points exceed 2^%d", a, kFftMaxLogTotal);
    const int a2 = a / 2, a1 = a - a2;  // n = n1 * L2 + n2, k = k1 + L1 * k2
    const long L1 = 1L << a1, L2 = 1L << a2;
    const float2 *tw1, *tw2, *twt;
    if (int rc = twiddles(call, a1, &tw1)) return rc;
    if (int rc = twiddles(call, a2, &tw2)) return rc;
    if (int rc = twiddles(call, a, &twt)) return rc;
    // columns: for each n2, L1 points n1 -> k1, times W_L^(n2 k1), in place at [k1 * L2 + n2]
    int C1 = (1 << kFftMaxLog) >> a1;
    long nt1 = n_sig * L2;
    if (int rc = launch(fft_lds_kernel, "fft_lds_kernel launch (columns)", dim3((unsigned)((nt1 + C1 - 1) / C1)), dim3(256), 0, st, buf, buf,
                        a1, C1, nt1, L2, L, 1L, L2, 1L, L2, tw1, dir, premul, twt, L - 1))
        return rc;
    // rows: for each k1, L2 points n2 -> k2, to [k1 + L1 * k2]
    int C2 = (1 << kFftMaxLog) >> a2;
    long nt2 = n_sig * L1;
    if (int rc = launch(fft_lds_kernel, "fft_lds_kernel launch (rows)", dim3((unsigned)((nt2 + C2 - 1) / C2)), dim3(256), 0, st, buf, tmp, a2,
                        C2, nt2, L1, L, L2, 1L, 1L, L1, tw2, dir, (const float2 *)nullptr, (const float2 *)nullptr, 0L))
        return rc;
    *result = tmp;
    return IIV_OK;
}

long bluestein_m(long L)
{
    long M = 1;
    while (M < 2 * L - 1) M <<= 1;
    return M;
}

bool is_pow2(long L) { return L > 0 && (L & (L - 1)) == 0; }

// the points the transforms of an L-point DFT run on: L itself, or Bluestein's M
long transform_points(long L) { return is_pow2(L) ? L : bluestein_m(L); }

// The chirp of an L-point DFT of sign dir, and the filter's spectrum FFT_M(conj chirp) / M (the inverse FFT of
// FFT_M(a) * bhat is then the circular convolution), both in the group's scope.
int bluestein_tables(Scratch &call, Scratch &group, long L, int dir, const float2 **chirp, const float2 **bhat)
{
    const long M = bluestein_m(L);
    float2 *c = nullptr, *d = nullptr, *t = nullptr, *res = nullptr;
    if (int rc = group.alloc(&c, (size_t)L, "hipMallocAsync(chirp)")) return rc;
    if (int rc = group.alloc(&d, (size_t)M, "hipMallocAsync(chirp spectrum)")) return rc;
    if (int rc = group.alloc(&t, (size_t)M, "hipMallocAsync(chirp spectrum)")) return rc;
    if (int rc = launch(chirp_kernel, "chirp_kernel launch", dim3((unsigned)((L + 255) / 256)), dim3(256), 0, group.st, c, L, dir)) return rc;
    if (int rc = launch(bluestein_b_kernel, "bluestein_b_kernel launch", dim3((unsigned)((M + 255) / 256)), dim3(256), 0, group.st, d, L, M, dir))
        return rc;
    if (int rc = fft(call, d, t, log2_exact(M), 1, -1, nullptr, &res)) return rc;
    *chirp = c;
    *bhat = res;
    return IIV_OK;
}

// ---- the resample pipeline ------------------------------------------------------------------------------------------

// to_mono (audio.py:53-55: int16 -> float32, channel mean) of each job's nx frames, times the forward chirp (Bluestein)
// or as is, zero-padded to lf points: buf[j * lf + n]
__global__ __launch_bounds__(256) void mono_kernel(const int16_t *__restrict__ pcm, const Job *__restrict__ jobs, long nx,
                                                   long lf, const float2 *__restrict__ chirp, float2 *__restrict__ buf)
{
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    const Job jb = jobs[blockIdx.y];
    if (n >= lf) return;
    float2 v = make_float2(0.f, 0.f);
    if (n < nx) {
        const int16_t *p = pcm + jb.pcm_off + n * jb.channels;
        float sum = 0.f;
        for (int c = 0; c < jb.channels; c++) sum += (float)p[c];
        v.x = sum / (float)jb.channels;
        if (chirp) v = cmul(v, chirp[n]);
    }
    buf[(size_t)blockIdx.y * lf + n] = v;
}

// scipy.signal.resample's spectrum of num points from the nx-point rfft (bins k < nyq = min(num, nx) / 2 + 1, the even
// Nyquist bin doubled when downsampling and halved when upsampling), completed to the Hermitian spectrum irfft inverts
// (imaginary parts of bin 0 and of an even num's bin num/2 dropped), times the inverse chirp (Bluestein) or as is,
// zero-padded to li points.  X[k] = spec[j * ls + k], times fchirp[k] when the forward transform was a Bluestein one.
__global__ __launch_bounds__(256) void spectrum_kernel(const float2 *__restrict__ spec, long ls, const float2 *__restrict__ fchirp,
                                                       long nx, long num, long li, const float2 *__restrict__ ichirp,
                                                       float2 *__restrict__ buf)
{
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    const long j = blockIdx.y;
    if (k >= li) return;
    float2 v = make_float2(0.f, 0.f);
    if (k < num) {
        const long N = num < nx ? num : nx;
        const long nyq = N / 2 + 1;
        const bool mirror = k > num / 2;
        const long kk = mirror ? num - k : k;
        if (kk < nyq) {
            v = spec[(size_t)j * ls + kk];
            if (fchirp) v = cmul(v, fchirp[kk]);
            if (N % 2 == 0 && kk == N / 2) {
                if (num < nx) { v.x *= 2.f; v.y *= 2.f; }
                else if (nx < num) { v.x *= 0.5f; v.y *= 0.5f; }
            }
            if (kk == 0 || (num % 2 == 0 && kk == num / 2)) v.y = 0.f;
            if (mirror) v.y = -v.y;
        }
        if (ichirp) v = cmul(v, ichirp[k]);
    }
    buf[(size_t)j * li + k] = v;
}

// scale -> normalise -> truncate -> clip -> tick (audio.py:99-105, movie.py:104-107), or the float sample (normalisation)
__device__ inline uint8_t tick_of(float y, float norm)
{
    float a = y * norm * (1.0f / 1024.0f);   // y / 16384 * normalization * 16, the powers of two exact
    a = truncf(a);                           // astype(int)
    a = fminf(fmaxf(a, -15.f), 16.f);        // clip(-15, 16); NaN cannot reach here (norm is finite, checked)
    return (uint8_t)(2 * (int)a + 34);
}

__global__ __launch_bounds__(256) void finish_kernel(const float2 *__restrict__ res, long lr, const float2 *__restrict__ chirp,
                                                     long num, const Job *__restrict__ jobs, uint8_t *__restrict__ ticks,
                                                     float *__restrict__ fout)
{
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= num) return;
    const Job jb = jobs[blockIdx.y];
    float2 v = res[(size_t)blockIdx.y * lr + n];
    float y = chirp ? v.x * chirp[n].x - v.y * chirp[n].y : v.x;
    y *= jb.scale;
    if (fout)
        fout[jb.out_off + n] = y;
    else
        ticks[jb.out_off + n] = tick_of(y, jb.norm);
}

// orig_sr == target_sr: librosa returns the mono signal untouched (no resampling, no scale)
__global__ __launch_bounds__(256) void identity_kernel(const int16_t *__restrict__ pcm, const Job *__restrict__ jobs, long nx,
                                                       uint8_t *__restrict__ ticks, float *__restrict__ fout)
{
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    const Job jb = jobs[blockIdx.y];
    if (n >= nx) return;
    const int16_t *p = pcm + jb.pcm_off + n * jb.channels;
    float sum = 0.f;
    for (int c = 0; c < jb.channels; c++) sum += (float)p[c];
    float y = sum / (float)jb.channels;
    if (fout)
        fout[jb.out_off + n] = y;
    else
        ticks[jb.out_off + n] = tick_of(y, jb.norm);
}

// librosa.resample's output length (0.9.2: ratio = target / orig, n = int(ceil(n_in * ratio)), both float64)
long n_out(long n_in, int rate, int bitrate)
{
    if (rate == bitrate) return n_in;
    double ratio = (double)bitrate / (double)rate;
    return (long)ceil((double)n_in * ratio);
}

constexpr size_t kWorkspaceBytes = 1UL << 30;  // per work buffer; a group of jobs is cut into chunks that fit

// Every job of one (nx, num) group: mono -> FFT_nx -> spectrum -> IFFT_num -> finish (identity: mono -> finish).  jobs: host
// array.  The group's buffers and chirp tables are stream-ordered allocations freed when the group is enqueued, so the call
// does not synchronise and its memory does not grow with the number of distinct lengths in a batch.
int run_group(Scratch &call, const int16_t *d_pcm, long nx, long num, bool identity, const std::vector<Job> &jobs,
              uint8_t *d_ticks, float *d_fout)
{
    if (jobs.empty()) return IIV_OK;
    hipStream_t st = call.st;
    Scratch group(st);
    const long J = (long)jobs.size();
    Job *d_jobs = nullptr;
    if (int rc = group.alloc(&d_jobs, (size_t)J, "hipMallocAsync(jobs)")) return rc;
    IIV_HIP(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(Job) * J, hipMemcpyHostToDevice, st));
    if (identity) {
        for (long j0 = 0; j0 < J; j0 += 65535) {
            long jc = J - j0 < 65535 ? J - j0 : 65535;
            if (int rc = launch(identity_kernel, "identity_kernel launch", dim3((unsigned)((nx + 255) / 256), (unsigned)jc), dim3(256), 0, st,
                                d_pcm, d_jobs + j0, nx, d_ticks, d_fout))
                return rc;
        }
        return IIV_OK;
    }
    const bool fb = !is_pow2(nx), ib = !is_pow2(num);
    const long lf = transform_points(nx), li = transform_points(num);
    const long lmax = lf > li ? lf : li;
    const float2 *fchirp = nullptr, *fbhat = nullptr, *ichirp = nullptr, *ibhat = nullptr;
    if (fb)
        if (int rc = bluestein_tables(call, group, nx, -1, &fchirp, &fbhat)) return rc;
    if (ib)
        if (int rc = bluestein_tables(call, group, num, +1, &ichirp, &ibhat)) return rc;
    long jc = (long)(kWorkspaceBytes / (sizeof(float2) * (size_t)lmax));
    jc = jc < 1 ? 1 : (jc > 65535 ? 65535 : jc);
    jc = jc > J ? J : jc;
    float2 *w0 = nullptr, *w1 = nullptr;
    if (int rc = group.alloc(&w0, (size_t)lmax * jc, "hipMallocAsync(work)")) return rc;
    if (int rc = group.alloc(&w1, (size_t)lmax * jc, "hipMallocAsync(work)")) return rc;
    const int af = log2_exact(lf), ai = log2_exact(li);
    for (long j0 = 0; j0 < J; j0 += jc) {
        const long n = J - j0 < jc ? J - j0 : jc;
        float2 *r = nullptr, *other;
        if (int rc = launch(mono_kernel, "mono_kernel launch", dim3((unsigned)((lf + 255) / 256), (unsigned)n), dim3(256), 0, st, d_pcm,
                            d_jobs + j0, nx, lf, fchirp, w0))
            return rc;
        if (int rc = fft(call, w0, w1, af, n, -1, nullptr, &r)) return rc;
        if (fb) {   // Bluestein: the convolution with the chirp, the inverse FFT of the product with the filter's spectrum
            other = r == w0 ? w1 : w0;
            if (int rc = fft(call, r, other, af, n, +1, fbhat, &r)) return rc;
        }
        other = r == w0 ? w1 : w0;
        if (int rc = launch(spectrum_kernel, "spectrum_kernel launch", dim3((unsigned)((li + 255) / 256), (unsigned)n), dim3(256), 0, st, r, lf,
                            fchirp, nx, num, li, ichirp, other))
            return rc;
        r = other;
        other = r == w0 ? w1 : w0;
        if (int rc = fft(call, r, other, ai, n, ib ? -1 : +1, nullptr, &r)) return rc;
        if (ib) {
            other = r == w0 ? w1 : w0;
            if (int rc = fft(call, r, other, ai, n, +1, ibhat, &r)) return rc;
        }
        if (int rc = launch(finish_kernel, "finish_kernel launch", dim3((unsigned)((num + 255) / 256), (unsigned)n), dim3(256), 0, st, r, li, ichirp,
                            num, d_jobs + j0, d_ticks, d_fout))
            return rc;
    }
    return IIV_OK;
}

// the jobs of one call, grouped by (nx, num); identity: rate == bitrate, grouped by length.  Every transform size is
// checked before anything is launched: a call either runs whole or is refused.
int run_jobs(const int16_t *d_pcm, const std::map<std::pair<long, long>, std::vector<Job>> &groups,
             const std::map<long, std::vector<Job>> &identity, uint8_t *d_ticks, float *d_fout, hipStream_t st)
{
    for (auto &g : groups)
        for (long L : {g.first.first, g.first.second})
            if (transform_points(L) > (1L << kFftMaxLogTotal))
                return set_error(IIV_ERR_INVALID, "audio: a %ld-point DFT needs a %ld-point transform, more than the 2^%d this "
                                 "library runs (DESIGN.md 10: shorter decode blocks, or a shorter normalisation prefix)",
                                 L, transform_points(L), kFftMaxLogTotal);
    Scratch call(st);
    for (auto &g : identity)
        if (int rc = run_group(call, d_pcm, g.first, g.first, true, g.second, d_ticks, d_fout)) return rc;
    for (auto &g : groups)
        if (int rc = run_group(call, d_pcm, g.first.first, g.first.second, false, g.second, d_ticks, d_fout)) return rc;
    return IIV_OK;
}

hipError_t have_device()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    return e != hipSuccess ? e : (n > 0 ? hipSuccess : hipErrorNoDevice);
}

int check_streams(int n_streams, const int16_t *d_pcm, size_t pcm_stride, const long *n_frames, const int *channels,
                  const int *rate, int bitrate)
{
    if (n_streams < 0 || n_streams > 65535 || (n_streams > 0 && (!d_pcm || !n_frames || !channels || !rate)))
        return set_error(IIV_ERR_INVALID, "audio: bad stream arrays");
    if (bitrate <= 0) return set_error(IIV_ERR_INVALID, "audio: bitrate must be > 0");
    for (int s = 0; s < n_streams; s++) {
        if (n_frames[s] < 0 || channels[s] < 1 || channels[s] > 64 || rate[s] <= 0)
            return set_error(IIV_ERR_INVALID, "audio: stream %d: n_frames %ld, channels %d, rate %d", s, n_frames[s], channels[s],
                             rate[s]);
        if ((size_t)n_frames[s] * (size_t)channels[s] > pcm_stride)
            return set_error(IIV_ERR_INVALID, "audio: stream %d: %ld frames x %d channels exceed pcm_stride %zu", s, n_frames[s],
                             channels[s], pcm_stride);
    }
    return IIV_OK;
}

// audio.py:62-66: blocks of kRawBlockFrames frames are read until more than 10 MiB are held
long prefix_frames(long n_frames, int channels)
{
    long bpb = kRawBlockFrames * 2 * channels;
    long blocks = kPrefixBytes / bpb + 1;
    long p = blocks * kRawBlockFrames;
    return p < n_frames ? p : n_frames;
}

// ---- radix select (the normalisation's percentiles) -----------------------------------------------------------------

__device__ inline uint32_t float_key(float f)
{
    uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ inline float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// four order statistics per stream: histogram of the next 8-bit digit of every key that matches the prefix so far
__global__ __launch_bounds__(256) void select_hist_kernel(const float *__restrict__ y, const long *__restrict__ off,
                                                          const long *__restrict__ len, const uint32_t *__restrict__ prefix,
                                                          int shift, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t h[4][256];
    const int s = blockIdx.y;
    for (int i = threadIdx.x; i < 1024; i += 256) (&h[0][0])[i] = 0;
    __syncthreads();
    const uint32_t hi_mask = shift == 24 ? 0u : ~((1u << (shift + 8)) - 1u);
    uint32_t p[4];
    for (int q = 0; q < 4; q++) p[q] = prefix[s * 4 + q];
    const long n = len[s];
    const float *ys = y + off[s];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        uint32_t k = float_key(ys[i]);
        for (int q = 0; q < 4; q++)
            if (((k ^ p[q]) & hi_mask) == 0) atomicAdd(&h[q][(k >> shift) & 255], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 1024; i += 256) {
        uint32_t v = (&h[0][0])[i];
        if (v) atomicAdd(&hist[(size_t)s * 1024 + i], v);
    }
}

// one thread per (stream, statistic): pick the digit the rank falls in
__global__ __launch_bounds__(64) void select_pick_kernel(int n_streams, int shift, uint32_t *__restrict__ hist,
                                                         uint32_t *__restrict__ prefix, uint32_t *__restrict__ rank)
{
    int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_streams * 4) return;
    uint32_t *h = hist + (size_t)i * 256;
    uint32_t r = rank[i], cum = 0;
    int d = 255;
    for (int b = 0; b < 256; b++) {
        if (cum + h[b] > r) { d = b; break; }
        cum += h[b];
    }
    rank[i] = r - cum;
    prefix[i] |= (uint32_t)d << shift;
    for (int b = 0; b < 256; b++) h[b] = 0;
}

__global__ void select_values_kernel(int n, const uint32_t *__restrict__ prefix, float *__restrict__ out)
{
    int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) out[i] = key_float(prefix[i]);
}

}  // namespace

}  // namespace iiv

using namespace iiv;

extern "C" {

long iiv_audio_tick_count(long n_frames, int rate, int bitrate, long block_frames)
{
    if (n_frames < 0 || rate <= 0 || bitrate <= 0 || block_frames <= 0)
        return set_error(IIV_ERR_INVALID, "audio_tick_count: n_frames >= 0, rate, bitrate, block_frames > 0");
    if (rate == bitrate) return n_frames;
    long full = n_frames / block_frames, rem = n_frames % block_frames;
    return full * n_out(block_frames, rate, bitrate) + (rem ? n_out(rem, rate, bitrate) : 0);
}

int iiv_audio_ticks(int n_streams, const int16_t *d_pcm, size_t pcm_stride, const long *n_frames, const int *channels,
                    const int *rate, int bitrate, long block_frames, const double *normalization, uint8_t *d_ticks,
                    size_t ticks_stride, long *n_ticks, void *stream)
{
    if (int rc = check_streams(n_streams, d_pcm, pcm_stride, n_frames, channels, rate, bitrate)) return rc;
    if (block_frames <= 0) return set_error(IIV_ERR_INVALID, "audio_ticks: block_frames must be > 0");
    if (n_streams > 0 && (!normalization || !d_ticks)) return set_error(IIV_ERR_INVALID, "audio_ticks: normalization / d_ticks NULL");
    IIV_HIP(have_device());
    std::map<std::pair<long, long>, std::vector<Job>> groups;
    std::map<long, std::vector<Job>> identity;
    for (int s = 0; s < n_streams; s++) {
        const double nm = normalization[s];
        if (!(nm != 0.0) || !isfinite(nm))
            return set_error(IIV_ERR_INVALID, "audio_ticks: stream %d: normalization %g (zero or not finite: a silent prefix?)", s, nm);
        long nt = iiv_audio_tick_count(n_frames[s], rate[s], bitrate, block_frames);
        if (nt < 0) return (int)nt;
        if ((size_t)nt > ticks_stride)
            return set_error(IIV_ERR_INVALID, "audio_ticks: stream %d has %ld ticks > ticks_stride %zu", s, nt, ticks_stride);
        if (n_ticks) n_ticks[s] = nt;
        const long base_pcm = (long)((size_t)s * pcm_stride), base_out = (long)((size_t)s * ticks_stride);
        if (rate[s] == bitrate) {
            if (n_frames[s] > 0) identity[n_frames[s]].push_back(Job{base_pcm, base_out, channels[s], 0.f, (float)nm});
            continue;
        }
        const double ratio = (double)bitrate / (double)rate[s];
        long out = 0;
        for (long f = 0; f < n_frames[s]; f += block_frames) {
            long nx = n_frames[s] - f < block_frames ? n_frames[s] - f : block_frames;
            long num = n_out(nx, rate[s], bitrate);
            float scale = (float)(1.0 / ((double)nx * sqrt(ratio)));
            groups[{nx, num}].push_back(Job{base_pcm + f * channels[s], base_out + out, channels[s], scale, (float)nm});
            out += num;
        }
    }
    return run_jobs(d_pcm, groups, identity, d_ticks, nullptr, (hipStream_t)stream);
}

int iiv_audio_resample(int n_streams, const int16_t *d_pcm, size_t pcm_stride, const long *n_frames, const int *channels,
                       const int *rate, int bitrate, float *d_out, size_t out_stride, long *n_out_samples, void *stream)
{
    if (int rc = check_streams(n_streams, d_pcm, pcm_stride, n_frames, channels, rate, bitrate)) return rc;
    if (n_streams > 0 && !d_out) return set_error(IIV_ERR_INVALID, "audio_resample: d_out NULL");
    IIV_HIP(have_device());
    std::map<std::pair<long, long>, std::vector<Job>> groups;
    std::map<long, std::vector<Job>> identity;
    for (int s = 0; s < n_streams; s++) {
        long nx = n_frames[s], num = n_out(nx, rate[s], bitrate);
        if ((size_t)num > out_stride)
            return set_error(IIV_ERR_INVALID, "audio_resample: stream %d has %ld samples > out_stride %zu", s, num, out_stride);
        if (n_out_samples) n_out_samples[s] = num;
        Job jb{(long)((size_t)s * pcm_stride), (long)((size_t)s * out_stride), channels[s], 0.f, 0.f};
        if (nx == 0) continue;
        if (rate[s] == bitrate) {
            identity[nx].push_back(jb);
        } else {
            jb.scale = (float)(1.0 / ((double)nx * sqrt((double)bitrate / (double)rate[s])));
            groups[{nx, num}].push_back(jb);
        }
    }
    return run_jobs(d_pcm, groups, identity, nullptr, d_out, (hipStream_t)stream);
}

int iiv_audio_normalization(int n_streams, const int16_t *d_pcm, size_t pcm_stride, const long *n_frames, const int *channels,
                            const int *rate, int bitrate, double *normalization, void *stream)
{
    if (int rc = check_streams(n_streams, d_pcm, pcm_stride, n_frames, channels, rate, bitrate)) return rc;
    if (n_streams > 0 && !normalization) return set_error(IIV_ERR_INVALID, "audio_normalization: normalization NULL");
    IIV_HIP(have_device());
    if (n_streams == 0) return IIV_OK;
    hipStream_t st = (hipStream_t)stream;
    std::vector<long> pf(n_streams), ns(n_streams), off(n_streams);
    long total = 0, mx = 0;
    for (int s = 0; s < n_streams; s++) {
        pf[s] = prefix_frames(n_frames[s], channels[s]);
        ns[s] = n_out(pf[s], rate[s], bitrate);
        if (ns[s] < 1) return set_error(IIV_ERR_INVALID, "audio_normalization: stream %d is empty", s);
        off[s] = total;
        total += ns[s];
        mx = ns[s] > mx ? ns[s] : mx;
    }
    // the prefixes, decoded as one block each (audio.py:67), side by side: stream s at y + off[s]
    DeviceBuf<float> d_y;
    if (int rc = d_y.alloc((size_t)total, "hipMalloc(prefixes)")) return rc;
    std::map<std::pair<long, long>, std::vector<Job>> groups;
    std::map<long, std::vector<Job>> identity;
    for (int s = 0; s < n_streams; s++) {
        Job jb{(long)((size_t)s * pcm_stride), off[s], channels[s], 0.f, 0.f};
        if (rate[s] == bitrate) {
            identity[pf[s]].push_back(jb);
        } else {
            jb.scale = (float)(1.0 / ((double)pf[s] * sqrt((double)bitrate / (double)rate[s])));
            groups[{pf[s], ns[s]}].push_back(jb);
        }
    }
    if (int rc = run_jobs(d_pcm, groups, identity, nullptr, d_y, st)) return rc;
    // np.percentile(a, [0.5, 99.5]) (linear): ranks floor(q (n-1)) and the next one, for both q
    std::vector<uint32_t> rank(4 * (size_t)n_streams);
    std::vector<double> frac(2 * (size_t)n_streams);
    for (int s = 0; s < n_streams; s++) {
        for (int h = 0; h < 2; h++) {
            double vi = (h ? 0.995 : 0.005) * (double)(ns[s] - 1);
            long lo = (long)floor(vi);
            long hi = lo + 1 < ns[s] ? lo + 1 : ns[s] - 1;
            rank[s * 4 + 2 * h] = (uint32_t)lo;
            rank[s * 4 + 2 * h + 1] = (uint32_t)hi;
            frac[s * 2 + h] = vi - (double)lo;
        }
    }
    DeviceBuf<uint32_t> d_sel;   // [hist n*1024][prefix n*4][rank n*4]
    DeviceBuf<float> d_val;
    DeviceBuf<long> d_meta;      // [off n][len n]
    std::vector<float> val(4 * (size_t)n_streams);
    if (int rc = d_sel.alloc((size_t)n_streams * 1032, "hipMalloc(select)")) return rc;
    if (int rc = d_val.alloc(4 * (size_t)n_streams, "hipMalloc(select values)")) return rc;
    std::vector<long> meta(2 * (size_t)n_streams);
    for (int s = 0; s < n_streams; s++) meta[s] = off[s], meta[n_streams + s] = ns[s];
    if (int rc = d_meta.alloc(2 * (size_t)n_streams, "hipMalloc(select meta)")) return rc;
    uint32_t *hist = d_sel, *prefix = d_sel + (size_t)n_streams * 1024, *drank = prefix + (size_t)n_streams * 4;
    IIV_HIP(hipMemsetAsync(d_sel, 0, sizeof(uint32_t) * (size_t)n_streams * 1028, st));
    IIV_HIP(hipMemcpyAsync(drank, rank.data(), sizeof(uint32_t) * 4 * n_streams, hipMemcpyHostToDevice, st));
    IIV_HIP(hipMemcpyAsync(d_meta, meta.data(), sizeof(long) * 2 * n_streams, hipMemcpyHostToDevice, st));
    unsigned gx = (unsigned)((mx + 255) / 256);
    gx = gx > 1024 ? 1024 : gx;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (int rc = launch(select_hist_kernel, "select_hist_kernel launch", dim3(gx, (unsigned)n_streams), dim3(256), 0, st, d_y, d_meta,
                         d_meta + n_streams, prefix, shift, hist))
            return rc;
        if (int rc = launch(select_pick_kernel, "select_pick_kernel launch", dim3((unsigned)((4 * n_streams + 63) / 64)), dim3(64), 0, st, n_streams,
                         shift, hist, prefix, drank))
            return rc;
    }
    if (int rc = launch(select_values_kernel, "select_values_kernel launch", dim3((unsigned)((4 * n_streams + 63) / 64)), dim3(64), 0, st,
                     4 * n_streams, prefix, d_val))
        return rc;
    IIV_HIP(hipMemcpyAsync(val.data(), d_val, sizeof(float) * 4 * n_streams, hipMemcpyDeviceToHost, st));
    IIV_HIP(hipStreamSynchronize(st));   // (the owners free behind it)
    for (int s = 0; s < n_streams; s++) {
        double m = 0.0;
        for (int h = 0; h < 2; h++) {
            double a = val[s * 4 + 2 * h], b = val[s * 4 + 2 * h + 1], t = frac[s * 2 + h];
            double p = a + (b - a) * t;   // numpy's linear interpolation
            m = fabs(p) > m ? fabs(p) : m;
        }
        normalization[s] = 16384.0 / m;   // audio.py:70 (inf for a silent prefix)
    }
    return IIV_OK;
}

}  // extern "C"
