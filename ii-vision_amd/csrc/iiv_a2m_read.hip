// iiv_a2m_read.hip -- reading an opcode stream (".a2m"): check it as written, decode it back to the encoder's records,
// replay it to the screen memory a player holds after k opcodes.  include/iivision.h section f9 is the specification;
// tests/a2m_model.py restates it in numpy; DESIGN.md 15.
//
// The layout is closed form (iiv_a2m_layout.h), so every slot is found without walking the stream: scan and decode run
// one thread per slot, as emit_kernel does, and replay is a last-writer-wins reduction per screen byte in LDS.
#include "iiv_host.h"
#include "iiv_a2m_layout.h"

#include <new>
#include <vector>

struct iiv_a2m_reader {
    iiv::DeviceBuf<uint16_t> inv;   // [65536] address -> tick index * 32 + page - 32, kInvAck, kInvTerminate, kInvNone
    uint16_t ack = 0, terminate = 0;
};

namespace iiv {

constexpr uint32_t kInvAck = 1024, kInvTerminate = 1025, kInvNone = 0xffff;
constexpr unsigned long long kNoOffence = ~0ull;   // the running minimum of position * 8 + status while a scan is in flight

// ---- what the three kernels share --------------------------------------------------------------------------------------

// the slot at byte p of stream b: its address looked up (< 1024: a tick opcode), its content byte and four offsets
struct Slot {
    uint32_t what, content, off[4];
};

__device__ static inline uint32_t slot_address(const uint8_t *__restrict__ b, size_t p, const uint16_t *__restrict__ inv)
{
    return inv[(uint32_t)b[p] << 8 | b[p + 1]];
}

__device__ static inline Slot slot_read(const uint8_t *__restrict__ b, size_t p, const uint16_t *__restrict__ inv)
{
    Slot s;
    s.what = slot_address(b, p, inv);
    s.content = b[p + 2];
    for (int i = 0; i < 4; i++) s.off[i] = b[p + 3 + i];
    return s;
}

// bank of opcode k: bit 0 of the bank byte of the last ACK before it (ACK j ends block j: bytes 2048 (j + 1) - 4 ..)
__device__ static inline uint32_t slot_bank(const uint8_t *__restrict__ b, long k)
{
    return k < 291 ? 0u : b[2048 * (size_t)(1 + (k - 291) / 292) - 2] & 1u;
}

__device__ static inline bool usable_length(long long L, size_t stride) { return L > 0 && L % 2048 == 0 && (size_t)L <= stride; }

__device__ static inline void offence(unsigned long long *key, size_t position, int status)
{
    atomicMin(key, (unsigned long long)position * 8 + (unsigned)status);
}

// ---- scan ----------------------------------------------------------------------------------------------------------------
// While the scan runs, info[s] = {-, mode, running minimum of n_ops, running minimum of the offence key}; both minima are of
// values that depend on the bytes alone, so the result does not depend on the order in which threads arrive.

__global__ __launch_bounds__(256) void scan_init_kernel(int n_streams, const uint8_t *__restrict__ bytes, size_t stride,
                                                        const long long *__restrict__ lengths, long long *__restrict__ info)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_streams) return;
    const long long L = lengths[s];
    long long *o = info + (size_t)s * 4;
    if (!usable_length(L, stride)) {
        o[0] = IIV_A2M_BAD_LENGTH, o[1] = 0, o[2] = 0, o[3] = (long long)(0 * 8 + IIV_A2M_BAD_LENGTH);
        return;
    }
    const uint8_t *b = bytes + (size_t)s * stride;
    unsigned long long key = kNoOffence;
    for (int i = 5; i >= 0; i--)
        if (b[i] != 0xff) key = (unsigned long long)i * 8 + IIV_A2M_BAD_HEADER;
    if (key == kNoOffence && b[6] > 1) key = 6 * 8 + IIV_A2M_BAD_HEADER;
    o[0] = 0, o[1] = b[6], o[2] = slot_count((size_t)L), o[3] = (long long)key;
}

// n_ops: the first slot whose address is no tick opcode's
__global__ __launch_bounds__(256) void scan_slots_kernel(unsigned blocks_per_stream, const uint8_t *__restrict__ bytes, size_t stride,
                                                         const long long *__restrict__ lengths, const uint16_t *__restrict__ inv,
                                                         long long *__restrict__ info)
{
    const unsigned s = blockIdx.x / blocks_per_stream;
    const long k = (long)(blockIdx.x % blocks_per_stream) * 256 + threadIdx.x;
    const long long L = lengths[s];
    if (!usable_length(L, stride) || k >= slot_count((size_t)L)) return;
    if (slot_address(bytes + (size_t)s * stride, tick_offset(k), inv) >= 1024) atomicMin(&info[(size_t)s * 4 + 2], (long long)k);
}

// the ACKs before slot n_ops, slot n_ops itself, and what follows it
__global__ __launch_bounds__(256) void scan_check_kernel(unsigned blocks_per_stream, const uint8_t *__restrict__ bytes, size_t stride,
                                                         const long long *__restrict__ lengths, const uint16_t *__restrict__ inv,
                                                         uint32_t ack_addr, long long *__restrict__ info)
{
    const unsigned s = blockIdx.x / blocks_per_stream;
    const long k = (long)(blockIdx.x % blocks_per_stream) * 256 + threadIdx.x;
    const long long L = lengths[s];
    if (!usable_length(L, stride)) return;
    const uint8_t *b = bytes + (size_t)s * stride;
    const long n_ops = (long)info[(size_t)s * 4 + 2], slots = slot_count((size_t)L);
    unsigned long long *key = reinterpret_cast<unsigned long long *>(info + (size_t)s * 4 + 3);
    if (k < n_ops) {
        const size_t p = tick_offset(k) + 7;
        if (p % 2048 == 2044) {
            if (b[p] != (ack_addr >> 8)) offence(key, p, IIV_A2M_BAD_ACK);
            else if (b[p + 1] != (ack_addr & 0xff)) offence(key, p + 1, IIV_A2M_BAD_ACK);
            else if ((b[p + 2] | 1) != 0x55) offence(key, p + 2, IIV_A2M_BAD_ACK);
            else if (b[p + 3] != 0xff) offence(key, p + 3, IIV_A2M_BAD_ACK);
        }
    }
    const size_t pt = tick_offset(n_ops);
    if (n_ops >= slots) {
        if (k == 0) offence(key, pt, IIV_A2M_NO_TERMINATE);
        return;
    }
    if (k == 0) {
        if (slot_address(b, pt, inv) != kInvTerminate) offence(key, pt, IIV_A2M_BAD_ADDRESS);
        const size_t end = (pt + 2 + 2047) / 2048 * 2048;   // (P(n) + 2 is never on a boundary itself)
        if ((size_t)L != end) offence(key, end, IIV_A2M_BAD_PADDING);
    }
    for (size_t i = pt + 2 + (size_t)k; i < (size_t)L; i += (size_t)blocks_per_stream * 256)
        if (b[i]) {
            offence(key, i, IIV_A2M_BAD_PADDING);   // (this thread's later bytes are at higher positions)
            break;
        }
}

__global__ __launch_bounds__(256) void scan_finish_kernel(int n_streams, long long *__restrict__ info)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_streams) return;
    long long *o = info + (size_t)s * 4;
    const unsigned long long key = (unsigned long long)o[3];
    o[0] = key == kNoOffence ? IIV_A2M_OK : (long long)(key & 7);
    o[3] = key == kNoOffence ? 0 : (long long)(key >> 3);
}

// ---- decode --------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void decode_kernel(unsigned blocks_per_stream, long max_slots, const uint8_t *__restrict__ bytes,
                                                     size_t stride, const long long *__restrict__ info, const uint16_t *__restrict__ inv,
                                                     uint8_t *__restrict__ ops, size_t ops_stride, uint8_t *__restrict__ ticks,
                                                     uint8_t *__restrict__ banks, size_t ticks_stride)
{
    const unsigned s = blockIdx.x / blocks_per_stream;
    const long k = (long)(blockIdx.x % blocks_per_stream) * 256 + threadIdx.x;
    long long n_ops = info[(size_t)s * 4 + 2];
    n_ops = n_ops < max_slots ? n_ops : max_slots;   // (a caller's d_info cannot take a read past the stream's stride)
    if (k >= n_ops) return;
    const uint8_t *b = bytes + (size_t)s * stride;
    const Slot t = slot_read(b, tick_offset(k), inv);
    if (t.what >= 1024) return;                      // (not what a scan's n_ops covers)
    uint8_t *q = ops + (size_t)s * ops_stride + (size_t)k * 6;
    q[0] = (uint8_t)(32 + (t.what & 31));
    q[1] = (uint8_t)t.content;
    for (int i = 0; i < 4; i++) q[2 + i] = (uint8_t)t.off[i];
    ticks[(size_t)s * ticks_stride + k] = (uint8_t)(4 + 2 * (t.what >> 5));
    banks[(size_t)s * ticks_stride + k] = (uint8_t)slot_bank(b, k);
}

// ---- replay --------------------------------------------------------------------------------------------------------------
// One workgroup per stream.  Its 2 x 8 KiB of screen memory live in LDS, and beside every screen byte a 32-bit stamp
// (sequence << 8 | content) that the opcodes of the current window race for with atomicMax: the opcode latest in stream order
// has the largest sequence and wins, whichever lane or wave gets there first, and an opcode that names an offset twice writes
// the same stamp twice.  A fold moves every non-zero stamp's content into the screen and clears the stamp; it comes at every
// snapshot boundary and at least every kReplayFold opcodes, and the sequence restarts at 1 behind it (so 24 bits never run
// out and a zero stamp always means "not written in this window").
constexpr int kReplayThreads = 512;
constexpr long kReplayFold = 4096;   // opcodes between two folds at most; <= 2^15
static_assert(kReplayFold <= (1 << 15), "the fold interval is specified as at most 2^15 opcodes");

__device__ static inline void replay_fold(uint32_t *stamps_s, uint32_t *screen_s)
{
    __syncthreads();
    for (int w = threadIdx.x; w < 4096; w += kReplayThreads) {
        const uint4 st = reinterpret_cast<const uint4 *>(stamps_s)[w];
        if ((st.x | st.y | st.z | st.w) == 0) continue;
        uint32_t v = screen_s[w];
        if (st.x) v = (v & 0xffffff00u) | (st.x & 0xff);
        if (st.y) v = (v & 0xffff00ffu) | (st.y & 0xff) << 8;
        if (st.z) v = (v & 0xff00ffffu) | (st.z & 0xff) << 16;
        if (st.w) v = (v & 0x00ffffffu) | (st.w & 0xff) << 24;
        screen_s[w] = v;
        reinterpret_cast<uint4 *>(stamps_s)[w] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
}

__global__ __launch_bounds__(kReplayThreads) void replay_kernel(long max_slots, const uint8_t *__restrict__ bytes, size_t stride,
                                                                const long long *__restrict__ info, const uint16_t *__restrict__ inv,
                                                                long first_snap, long snap_every, int n_snaps,
                                                                const uint8_t *__restrict__ init_main, const uint8_t *__restrict__ init_aux,
                                                                uint8_t *__restrict__ out_main, uint8_t *__restrict__ out_aux)
{
    __shared__ __attribute__((aligned(16))) uint32_t stamps_s[2 * 8192];   // [bank][page - 32][offset]
    __shared__ __attribute__((aligned(16))) uint32_t screen_s[2 * 2048];   // the same bytes, four to a word
    const size_t s = blockIdx.x;
    const uint8_t *b = bytes + s * stride;
    long n_ops = (long)info[s * 4 + 2];
    n_ops = n_ops < 0 ? 0 : n_ops < max_slots ? n_ops : max_slots;

    for (int w = threadIdx.x; w < 2048; w += kReplayThreads) {   // 8 bytes a lane
        const uint8_t *src = w < 1024 ? init_main : init_aux;
        reinterpret_cast<uint2 *>(screen_s)[w] =
            src ? *reinterpret_cast<const uint2 *>(src + s * 8192 + (size_t)(w & 1023) * 8) : make_uint2(0, 0);
    }
    for (int i = threadIdx.x; i < 2 * 8192; i += kReplayThreads) stamps_s[i] = 0;
    __syncthreads();

    long pos = 0;
    for (int j = 0; j < n_snaps; j++) {
        long target = n_ops;   // min(first_snap + j * snap_every, n_ops) without forming a product that overflows
        if (first_snap < n_ops) {
            if (j == 0) target = first_snap;
            else if (snap_every <= (n_ops - first_snap) / j) target = first_snap + (long)j * snap_every;
        }
        while (pos < target) {
            const long end = target - pos < kReplayFold ? target : pos + kReplayFold;
            for (long k = pos + threadIdx.x; k < end; k += kReplayThreads) {
                const Slot t = slot_read(b, tick_offset(k), inv);
                if (t.what >= 1024) continue;   // (not what a scan's n_ops covers: nothing is stored)
                uint32_t *row = stamps_s + slot_bank(b, k) * 8192 + (t.what & 31) * 256;
                const uint32_t stamp = (uint32_t)(k - pos + 1) << 8 | t.content;
                for (int i = 0; i < 4; i++) atomicMax(row + t.off[i], stamp);
            }
            replay_fold(stamps_s, screen_s);
            pos = end;
        }
        uint8_t *om = out_main + (s * n_snaps + j) * 8192, *oa = out_aux + (s * n_snaps + j) * 8192;
        for (int w = threadIdx.x; w < 2048; w += kReplayThreads) {   // 8 bytes a lane
            const uint2 v = reinterpret_cast<const uint2 *>(screen_s)[w];
            *reinterpret_cast<uint2 *>((w < 1024 ? om : oa) + (size_t)(w & 1023) * 8) = v;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------

static bool aligned8(const void *p) { return ((uintptr_t)p & 7) == 0; }

// the flattened (stream, block of 256 slots) grid of the one-thread-per-slot kernels; 0 if it does not fit a launch
static unsigned slot_grid(int n_streams, size_t stride, unsigned *blocks_per_stream)
{
    const long blocks = (slot_count(stride) + 255) / 256;
    if (blocks <= 0 || blocks * (long)n_streams > 0x7fffffffL) return 0;
    *blocks_per_stream = (unsigned)blocks;
    return (unsigned)(blocks * n_streams);
}

}  // namespace iiv

using namespace iiv;

extern "C" int iiv_a2m_reader_create(const uint16_t tick_addr[1024], uint16_t ack_addr, uint16_t terminate_addr, iiv_a2m_reader **out)
{
    if (!tick_addr || !out) return set_error(IIV_ERR_INVALID, "iiv_a2m_reader_create: NULL argument");
    *out = nullptr;
    std::vector<uint16_t> inv(65536, (uint16_t)kInvNone);
    for (uint32_t i = 0; i < 1024; i++) {
        if (inv[tick_addr[i]] != kInvNone)
            return set_error(IIV_ERR_INVALID, "iiv_a2m_reader_create: tick address 0x%04x appears twice", tick_addr[i]);
        inv[tick_addr[i]] = (uint16_t)i;
    }
    if (inv[ack_addr] != kInvNone || inv[terminate_addr] != kInvNone || ack_addr == terminate_addr)
        return set_error(IIV_ERR_INVALID, "iiv_a2m_reader_create: the ack and terminate addresses must differ from each other and from every tick address");
    inv[ack_addr] = (uint16_t)kInvAck;
    inv[terminate_addr] = (uint16_t)kInvTerminate;
    iiv_a2m_reader *r = new (std::nothrow) iiv_a2m_reader;
    if (!r) return set_error(IIV_ERR_OVERFLOW, "iiv_a2m_reader_create: out of memory");
    r->ack = ack_addr, r->terminate = terminate_addr;
    int rc = r->inv.alloc(65536, "hipMalloc(address table)");
    if (!rc) rc = hip_check(hipMemcpy(r->inv.get(), inv.data(), 65536 * sizeof(uint16_t), hipMemcpyHostToDevice), "copy address table");
    if (rc) {
        delete r;
        return rc;
    }
    *out = r;
    return IIV_OK;
}

extern "C" void iiv_a2m_reader_destroy(iiv_a2m_reader *reader) { delete reader; }

extern "C" long iiv_a2m_max_ops(size_t length) { return slot_count(length); }

extern "C" int iiv_a2m_scan(const iiv_a2m_reader *reader, int n_streams, const uint8_t *d_bytes, size_t stride, const int64_t *d_lengths,
                            int64_t *d_info, void *stream)
{
    unsigned bps = 0, grid = 0;
    if (!reader || n_streams < 0 || !d_bytes || !d_lengths || !d_info || stride < 2048 || !aligned8(d_lengths) || !aligned8(d_info) ||
        (n_streams && !(grid = slot_grid(n_streams, stride, &bps))))
        return set_error(IIV_ERR_INVALID, "iiv_a2m_scan: bad argument");
    if (n_streams == 0) return IIV_OK;
    hipStream_t st = (hipStream_t)stream;
    const long long *len = reinterpret_cast<const long long *>(d_lengths);
    long long *info = reinterpret_cast<long long *>(d_info);
    const unsigned per_stream = (unsigned)((n_streams + 255) / 256);
    if (int rc = launch(scan_init_kernel, "scan_init_kernel launch", dim3(per_stream), dim3(256), 0, st, n_streams, d_bytes, stride, len, info))
        return rc;
    if (int rc = launch(scan_slots_kernel, "scan_slots_kernel launch", dim3(grid), dim3(256), 0, st, bps, d_bytes, stride, len, reader->inv, info))
        return rc;
    if (int rc = launch(scan_check_kernel, "scan_check_kernel launch", dim3(grid), dim3(256), 0, st, bps, d_bytes, stride, len, reader->inv,
                        (uint32_t)reader->ack, info))
        return rc;
    return launch(scan_finish_kernel, "scan_finish_kernel launch", dim3(per_stream), dim3(256), 0, st, n_streams, info);
}

extern "C" int iiv_a2m_decode(const iiv_a2m_reader *reader, int n_streams, const uint8_t *d_bytes, size_t stride, const int64_t *d_info,
                              uint8_t *d_ops, size_t ops_stride, uint8_t *d_ticks, uint8_t *d_banks, size_t ticks_stride, void *stream)
{
    unsigned bps = 0, grid = 0;
    if (!reader || n_streams < 0 || !d_bytes || !d_info || !d_ops || !d_ticks || !d_banks || stride < 2048 || !aligned8(d_info) ||
        (n_streams && !(grid = slot_grid(n_streams, stride, &bps))))
        return set_error(IIV_ERR_INVALID, "iiv_a2m_decode: bad argument");
    const long max_slots = slot_count(stride);
    if (ops_stride < (size_t)max_slots * 6 || ticks_stride < (size_t)max_slots)
        return set_error(IIV_ERR_INVALID, "iiv_a2m_decode: ops_stride %zu / ticks_stride %zu hold fewer than iiv_a2m_max_ops(stride) = %ld opcodes",
                         ops_stride, ticks_stride, max_slots);
    if (n_streams == 0) return IIV_OK;
    return launch(decode_kernel, "a2m decode_kernel launch", dim3(grid), dim3(256), 0, (hipStream_t)stream, bps, max_slots, d_bytes, stride,
                  reinterpret_cast<const long long *>(d_info), reader->inv, d_ops, ops_stride, d_ticks, d_banks, ticks_stride);
}

extern "C" int iiv_a2m_replay(const iiv_a2m_reader *reader, int n_streams, const uint8_t *d_bytes, size_t stride, const int64_t *d_info,
                              long first_snap, long snap_every, int n_snaps, const uint8_t *d_init_main, const uint8_t *d_init_aux,
                              uint8_t *d_main, uint8_t *d_aux, void *stream)
{
    if (!reader || n_streams < 0 || !d_bytes || !d_info || !d_main || !d_aux || stride < 2048 || first_snap < 0 || snap_every < 1 ||
        n_snaps < 1 || !aligned8(d_info) || !aligned8(d_main) || !aligned8(d_aux) || !aligned8(d_init_main) || !aligned8(d_init_aux))
        return set_error(IIV_ERR_INVALID, "iiv_a2m_replay: bad argument");
    if (n_streams == 0) return IIV_OK;
    return launch(replay_kernel, "a2m replay_kernel launch", dim3((unsigned)n_streams), dim3(kReplayThreads), 0, (hipStream_t)stream,
                  slot_count(stride), d_bytes, stride, reinterpret_cast<const long long *>(d_info), reader->inv, first_snap, snap_every,
                  n_snaps, d_init_main, d_init_aux, d_main, d_aux);
}
