// iiv_encoder.hip -- the encoder object apart from its launches (iiv_encode.hip): creation and options, snapshots, the
// streams' state as the host reads and writes it, the read-outs (check, profile, launch forms, input statistics), and the
// C ABI of all of these.
#include "iiv_encoder.h"

#include <memory>

namespace iiv {

static void seed_by_array(uint32_t mt[624], const uint32_t *key, int n)
{
    mt[0] = 19650218u;
    for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    int i = 1, j = 0;
    for (int k = 624 > n ? 624 : n; k; k--) {
        mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
        i++; j++;
        if (i >= 624) { mt[0] = mt[623]; i = 1; }
        if (j >= n) j = 0;
    }
    for (int k = 623; k; k--) {
        mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
        i++;
        if (i >= 624) { mt[0] = mt[623]; i = 1; }
    }
    mt[0] = 0x80000000u;
}

static void seed_genrand(uint32_t mt[624], uint32_t s)
{
    mt[0] = s;
    for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
}

// Video.__init__ (video.py:21-62) for every stream: blank screen, zero priorities, both RNG
// streams at their seed-0 state (rng0 = mt_py | mt_np, 1248 words)
__global__ __launch_bounds__(256) void init_states_kernel(StreamState *__restrict__ states, const uint32_t *__restrict__ rng0)
{
    StreamState &S = states[blockIdx.x];
    uint2 *q = reinterpret_cast<uint2 *>(&S);
    const uint2 z = make_uint2(0, 0);
    for (size_t i = threadIdx.x; i < sizeof(StreamState) / 8; i += 256) q[i] = z;
    __syncthreads();
    for (int i = threadIdx.x; i < 624; i += 256) {
        S.mt_py[i] = rng0[i];
        S.mt_np[i] = rng0[624 + i];
    }
    if (threadIdx.x == 0) {
        S.mt_py_idx = 624;
        S.mt_np_idx = 624;
    }
}
static_assert(sizeof(StreamState) % 8 == 0, "StreamState is cleared 8 bytes at a time");

// The priorities as the host sees them (int32, StreamState::up) from the kernels' 16-bit copy, and back (iiv_stream.h):
// one workgroup per stream, before the host reads / after it has written them.
__global__ __launch_bounds__(256) void materialise_up_kernel(StreamState *__restrict__ states)
{
    StreamState &S = states[blockIdx.x];
    for (int i = threadIdx.x; i < 2 * 8192; i += 256) {
        const uint32_t v = S.up16[i >> 13][i & 8191];
        if (v != kUpBig) S.up[i >> 13][i & 8191] = (int32_t)v;
    }
}
__global__ __launch_bounds__(256) void compact_up_kernel(StreamState *__restrict__ states)
{
    StreamState &S = states[blockIdx.x];
    for (int i = threadIdx.x; i < 2 * 8192; i += 256) {
        const uint32_t u = (uint32_t)S.up[i >> 13][i & 8191];
        S.up16[i >> 13][i & 8191] = (uint16_t)(u < kUpBig ? u : kUpBig);
    }
}
static int materialise_up(Encoder *e, int s0, int n)
{
    if (int rc = launch(materialise_up_kernel, "materialise_up_kernel launch", dim3(n), dim3(256), 0, 0, e->d_states + s0)) return rc;
    return hip_check(hipDeviceSynchronize(), "materialise_up sync");
}

__global__ __launch_bounds__(256) void max_u16_kernel(const uint16_t *__restrict__ v, size_t n, uint32_t *__restrict__ result)
{
    uint32_t mx = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) mx = max(mx, (uint32_t)v[i]);
    for (int d = 1; d < 64; d <<= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(result, mx);
}

int encoder_create(int mode, const uint16_t *d_table, const uint16_t *d_store, const int32_t *dm, int n_streams,
                   iiv_encoder **out)
{
    if (!out) return set_error(IIV_ERR_INVALID, "iiv_encoder_create: out is NULL");
    if ((mode != kHGR && mode != kDHGR) || (!d_table && !dm) || !d_store || n_streams <= 0)
        return set_error(IIV_ERR_INVALID, "iiv_encoder_create: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_error(IIV_ERR_NO_DEVICE, "iiv_encoder_create: no HIP device");
    if (dm) {
        // every diff weight is a sum of <= MASKED_DOTS substitute costs; the kernels pack diff
        // weights and store values into 11-bit fields (iiv_stream.h)
        int mx = 0;
        for (int i = 0; i < 256; i++) {
            if (dm[i] < 0) return set_error(IIV_ERR_INVALID, "iiv_encoder_create: dm[%d] < 0", i);
            mx = dm[i] > mx ? dm[i] : mx;
        }
        if (mx * masked_dots(mode) > kMaxValue)
            return set_error(IIV_ERR_INVALID, "iiv_encoder_create: max(dm) * MASKED_DOTS = %d exceeds %d",
                             mx * masked_dots(mode), kMaxValue);
    }
    std::unique_ptr<iiv_encoder> e(new iiv_encoder);   // (released with everything it holds on every early return)
    e->mode = mode;
    e->n_streams = n_streams;
    e->d_table = d_table;
    e->d_store = d_store;
    e->dw_mode = dm ? IIV_DW_RECURRENCE : IIV_DW_TABLE;
    if (int rc = e->d_states.alloc((size_t)n_streams, "hipMalloc(stream states)")) return rc;
    if (int rc = e->d_result.alloc(2, "hipMalloc(result)")) return rc;
    if (n_streams >= kOrderMinStreams) {
        if (int rc = e->d_cost.alloc((size_t)n_streams, "hipMalloc(stream costs)")) return rc;
        IIV_HIP(hipMemset(e->d_cost, 0, sizeof(uint32_t) * (size_t)n_streams));
        if (int rc = e->d_perm.alloc((size_t)n_streams, "hipMalloc(stream order)")) return rc;
    }
    if (int rc = e->d_packed.alloc(4096, "hipMalloc(packed)")) return rc;
    // (the brief's staging struct: here, not on first use -- an allocation inside the asynchronous entry point would synchronise)
    if (int rc = e->d_brief.alloc(1, "hipMalloc(brief)")) return rc;
    if (int rc = e->seg_ev[0].create(hipEventDisableTiming, "event")) return rc;
    if (int rc = e->seg_ev[1].create(hipEventDisableTiming, "event")) return rc;
    if (int rc = e->d_tie_stats.alloc(3, "hipMalloc(tie statistics)")) return rc;
    IIV_HIP(hipMemset(e->d_tie_stats, 0, 3 * sizeof(unsigned long long)));
    if (int rc = e->h_tie_stats.alloc(3, hipHostMallocDefault, "hipHostMalloc(tie statistics)")) return rc;
    e->h_tie_stats[0] = e->h_tie_stats[1] = e->h_tie_stats[2] = 0;
    if (int rc = e->tie_ev.create(hipEventDisableTiming, "event")) return rc;
    // the table values must fit the 11-bit fields too (a caller-made table may not come from dm)
    uint32_t h_max = 0;
    IIV_HIP(hipMemset(e->d_result, 0, 8));
    const size_t n_store = (size_t)num_offsets(mode) << (content_bits(mode) + masked_bits(mode));
    uint32_t *d_max = (uint32_t *)e->d_result.get();
    if (int rc = launch(max_u16_kernel, "max_u16_kernel launch", dim3(1024), dim3(256), 0, 0, d_store, n_store, d_max)) return rc;
    if (!dm && d_table)
        if (int rc = launch(max_u16_kernel, "max_u16_kernel launch", dim3(4096), dim3(256), 0, 0, d_table,
                            (size_t)num_offsets(mode) << (2 * masked_bits(mode)), d_max))
            return rc;
    IIV_HIP(hipMemcpy(&h_max, e->d_result, 4, hipMemcpyDeviceToHost));
    if (h_max > (uint32_t)kMaxValue)
        return set_error(IIV_ERR_INVALID, "iiv_encoder_create: table value %u exceeds %d", h_max, kMaxValue);
    if (dm) {
        if (int rc = build_strings(mode, dm, e->d_strings, e->d_sub, 0)) return rc;
        if (mode == kHGR)
            if (int rc = build_hgr_dot_lut(e->d_hgr_dots, 0)) return rc;
        if (int rc = build_dw_piece_table(mode, e->d_sub, e->d_dw_pieces, 0)) return rc;
        if (int rc = e->d_left.alloc(split_entries(mode, 0), "hipMalloc(split left)")) return rc;
        if (int rc = e->d_right.alloc(split_entries(mode, 1), "hipMalloc(split right)")) return rc;
        if (int rc = build_split_tables(mode, e->d_strings, e->d_sub, e->d_left, e->d_right, 0)) return rc;
        // (the folded narrow form is compared with the caller's store table entry by entry: e->nt.exact)
        if (int rc = build_narrow_tables(mode, e->d_strings, e->d_sub, e->d_left, d_store, &e->nt, e->nt_storage, 0)) return rc;
    }
    // Video.__init__ (video.py:21-62); RNG streams default to random.seed(0) / np.random.seed(0)
    uint32_t rng0[1248], key0 = 0;
    seed_by_array(rng0, &key0, 1);
    seed_genrand(rng0 + 624, 0);
    DeviceBuf<uint32_t> d_rng0;
    if (int rc = d_rng0.alloc(1248, "hipMalloc(rng0)")) return rc;
    IIV_HIP(hipMemcpy(d_rng0, rng0, sizeof(rng0), hipMemcpyHostToDevice));
    if (e->d_perm)
        if (int rc = launch_order_streams(e->d_cost, n_streams, e->d_perm, 1, 0)) return rc;
    if (int rc = launch(init_states_kernel, "init_states_kernel launch", dim3(n_streams), dim3(256), 0, 0, e->d_states, d_rng0)) return rc;
    IIV_HIP(hipDeviceSynchronize());
    *out = e.release();
    return IIV_OK;
}

int encoder_snapshot(Encoder *e, int slot, hipStream_t st)
{
    if (!e || slot < 0 || slot > 1) return set_error(IIV_ERR_INVALID, "snapshot: null encoder or slot not 0 / 1");
    const size_t bytes = sizeof(StreamState) * (size_t)e->n_streams;
    DeviceBuf<StreamState> fresh;   // (the slot's first snapshot: the slot has it once the copy is under way)
    if (!e->d_snapshot[slot])
        if (int rc = fresh.alloc((size_t)e->n_streams, "hipMalloc(snapshot)")) return rc;
    IIV_HIP(hipMemcpyAsync(fresh ? fresh : e->d_snapshot[slot], e->d_states, bytes, hipMemcpyDeviceToDevice, st));
    if (fresh) e->d_snapshot[slot] = std::move(fresh);
    e->snap_gens[slot] = e->gens;
    return IIV_OK;
}

int encoder_rollback(Encoder *e, int slot, hipStream_t st)
{
    if (!e || slot < 0 || slot > 1 || !e->d_snapshot[slot]) return set_error(IIV_ERR_INVALID, "rollback: no snapshot in that slot");
    const size_t bytes = sizeof(StreamState) * (size_t)e->n_streams;
    IIV_HIP(hipMemcpyAsync(e->d_states, e->d_snapshot[slot], bytes, hipMemcpyDeviceToDevice, st));
    e->gens = e->snap_gens[slot];
    return IIV_OK;
}

int encoder_set_option(Encoder *e, int option, int value)
{
    if (!e) return set_error(IIV_ERR_INVALID, "set_option: null encoder");
    if (option == IIV_OPT_DIFF_WEIGHTS) {
        if (value == IIV_DW_TABLE && !e->d_table) return set_error(IIV_ERR_INVALID, "no table was given at creation");
        if ((value == IIV_DW_RECURRENCE || value == IIV_DW_SPLIT) && !e->d_strings)
            return set_error(IIV_ERR_INVALID, "no diff matrix was given at creation");
        if (value != IIV_DW_TABLE && value != IIV_DW_RECURRENCE && value != IIV_DW_SPLIT)
            return set_error(IIV_ERR_INVALID, "bad value");
        if (value == IIV_DW_SPLIT && !e->d_dwl) {  // built on first use: 4-5 MiB, a few hundred microseconds
            DeviceBuf<uint32_t> l, r;   // (the encoder has them once they are built)
            int rc = l.alloc(split_dw_entries(e->mode, 0), "hipMalloc(split diff weights, left)");
            if (!rc) rc = r.alloc(split_dw_entries(e->mode, 1), "hipMalloc(split diff weights, right)");
            if (!rc) rc = build_split_dw_tables(e->mode, e->d_strings, e->d_sub, l, r, 0);
            if (rc) return rc;
            IIV_HIP(hipDeviceSynchronize());
            e->d_dwl = std::move(l);
            e->d_dwr = std::move(r);
        }
        e->dw_mode = value;
        return IIV_OK;
    }
    if (option == IIV_OPT_PREFIX_SORT) {
        e->partial_sort = value ? 1 : 0;
        return IIV_OK;
    }
    if (option == IIV_OPT_GREEDY_KERNEL) {
        if (value != IIV_GREEDY_WAVE && value != IIV_GREEDY_WORKGROUP && value != IIV_GREEDY_AUTO && value != IIV_GREEDY_TEAM &&
            value != IIV_GREEDY_WAVE_SHARED && value != IIV_GREEDY_WAVE_PLAIN)
            return set_error(IIV_ERR_INVALID, "bad value");
        if ((value == IIV_GREEDY_WAVE || value == IIV_GREEDY_TEAM || value == IIV_GREEDY_WAVE_SHARED || value == IIV_GREEDY_WAVE_PLAIN) && !e->d_left)
            return set_error(IIV_ERR_INVALID, "the one-wave kernel reads the split store table, which is built from dm "
                                               "(none was given at creation)");
        if (value != IIV_GREEDY_WORKGROUP && value != IIV_GREEDY_AUTO && !e->nt.exact)
            return set_error(IIV_ERR_INVALID, "the split store table built from dm does not reproduce the store table given at creation: "
                                               "this encoder runs the dense-table workgroup kernel only");
        e->greedy_mode = value;
        return IIV_OK;
    }
    if (option == IIV_OPT_GREEDY_LDS_PAD) {
        if (value < 0 || value > 32768) return set_error(IIV_ERR_INVALID, "bad value");
        e->greedy_lds_pad = value;
        return IIV_OK;
    }
    if (option == IIV_OPT_CONTENT_CHOICE) {
        if (value != IIV_CONTENT_TARGET && value != IIV_CONTENT_JOINT && value != IIV_CONTENT_JOINT_SPLIT)
            return set_error(IIV_ERR_INVALID, "bad value");
        if (value != IIV_CONTENT_TARGET && !e->d_left)
            return set_error(IIV_ERR_INVALID, "the joint content choice reads the split store table, which is built "
                                               "from dm (none was given at creation)");
        // (a store table that the narrow form does not reproduce -- not the one dm yields -- leaves only the split-table form)
        if (value == IIV_CONTENT_JOINT && !e->nt.exact) value = IIV_CONTENT_JOINT_SPLIT;
        if (value == IIV_CONTENT_JOINT && !e->d_joint_l) {
            DeviceBuf<uint32_t> l, r;
            if (int rc = build_joint_tables(e->mode, e->nt, l, r, 0)) return rc;
            IIV_HIP(hipDeviceSynchronize());
            e->d_joint_l = std::move(l);
            e->d_joint_r = std::move(r);
        }
        if (value == IIV_CONTENT_JOINT_SPLIT && !e->d_left_t) {
            DeviceBuf<uint32_t> l, r;
            int rc = l.alloc(split_entries(e->mode, 0), "hipMalloc(split left, transposed)");
            if (!rc) rc = r.alloc(split_entries(e->mode, 1), "hipMalloc(split right, transposed)");
            if (!rc) rc = transpose_split_tables(e->mode, e->d_left, e->d_right, l, r, 0);
            if (rc) return rc;
            IIV_HIP(hipDeviceSynchronize());
            e->d_left_t = std::move(l);
            e->d_right_t = std::move(r);
        }
        e->content_choice = value;
        return IIV_OK;
    }
    if (option == IIV_OPT_FOURTH_OFFSET) {
        if (value != 0 && value != 1) return set_error(IIV_ERR_INVALID, "bad value");
        if (value && (!e->d_left || !e->nt.exact))
            return set_error(IIV_ERR_INVALID, "the fourth offset runs in the one-wave kernel, which reads the split store table "
                                               "built from dm (none was given at creation, or it does not reproduce the store table given)");
        e->fourth_offset = value;
        return IIV_OK;
    }
    if (option == IIV_OPT_STREAM_ORDER) {
        if (value != 0 && value != 1) return set_error(IIV_ERR_INVALID, "bad value");
        e->order_streams = value;
        return IIV_OK;
    }
    return set_error(IIV_ERR_INVALID, "unknown option %d", option);
}

static int state_item(int mode, int what, size_t &off, size_t &bytes, bool &writable)
{
    writable = true;
    switch (what) {
    case IIV_STATE_MEM_MAIN: off = offsetof(StreamState, mem[0]); bytes = 8192; return 0;
    case IIV_STATE_MEM_AUX:
        if (mode != kDHGR) return -1;
        off = offsetof(StreamState, mem[1]); bytes = 8192; return 0;
    case IIV_STATE_UP_MAIN: off = offsetof(StreamState, up[0]); bytes = 8192 * 4; return 0;
    case IIV_STATE_UP_AUX:
        if (mode != kDHGR) return -1;
        off = offsetof(StreamState, up[1]); bytes = 8192 * 4; return 0;
    case IIV_STATE_OUT_OF_WORK: off = offsetof(StreamState, out_of_work); bytes = 8; return 0;
    case IIV_STATE_COUNTERS: off = offsetof(StreamState, draws_py); bytes = 32; writable = false; return 0;
    case 100: off = offsetof(StreamState, stamps); bytes = 256; writable = false; return 0;  // diagnostic
    default: return -1;
    }
}

// where a StreamState keeps IIV_STATE_RNG_PY / IIV_STATE_RNG_NP: the block's 624 words, its index
struct RngOffsets { size_t mt, idx; };
static RngOffsets rng_offsets(int what)
{
    return what == IIV_STATE_RNG_PY ? RngOffsets{offsetof(StreamState, mt_py), offsetof(StreamState, mt_py_idx)}
                                    : RngOffsets{offsetof(StreamState, mt_np), offsetof(StreamState, mt_np_idx)};
}

int encoder_get_state(Encoder *e, int s, int what, void *buf, size_t bytes)
{
    if (!e || !buf || s < 0 || s >= e->n_streams) return set_error(IIV_ERR_INVALID, "get_state: bad argument");
    IIV_HIP(hipDeviceSynchronize());
    uint8_t *base = reinterpret_cast<uint8_t *>(e->d_states + s);
    if (what == IIV_STATE_RNG_PY || what == IIV_STATE_RNG_NP) {
        if (bytes != 625 * 4) return set_error(IIV_ERR_INVALID, "get_state: RNG state is 625 u32");
        const RngOffsets o = rng_offsets(what);
        IIV_HIP(hipMemcpy(buf, base + o.mt, 624 * 4, hipMemcpyDeviceToHost));
        IIV_HIP(hipMemcpy((uint8_t *)buf + 624 * 4, base + o.idx, 4, hipMemcpyDeviceToHost));
        return IIV_OK;
    }
    if (what == IIV_STATE_PACKED) {
        if (bytes != 4096 * 8) return set_error(IIV_ERR_INVALID, "get_state: packed is 32x128 u64");
        int rc = pack(e->mode, 1, base + offsetof(StreamState, mem[0]), base + offsetof(StreamState, mem[1]), e->d_packed, 0);
        if (!rc) rc = hip_check(hipMemcpy(buf, e->d_packed, 4096 * 8, hipMemcpyDeviceToHost), "copy packed");
        return rc;
    }
    size_t off, want;
    bool writable;
    if (state_item(e->mode, what, off, want, writable)) return set_error(IIV_ERR_INVALID, "get_state: unknown item %d", what);
    if (bytes != want) return set_error(IIV_ERR_INVALID, "get_state: item %d is %zu bytes, got %zu", what, want, bytes);
    if (what == IIV_STATE_UP_MAIN || what == IIV_STATE_UP_AUX)
        if (int rc = materialise_up(e, s, 1)) return rc;
    IIV_HIP(hipMemcpy(buf, base + off, bytes, hipMemcpyDeviceToHost));
    return IIV_OK;
}

// n consecutive streams starting at s0; buf = n items back to back
int encoder_set_state(Encoder *e, int s0, int n, int what, const void *buf, size_t bytes)
{
    if (!e || !buf || n <= 0 || s0 < 0 || s0 + n > e->n_streams) return set_error(IIV_ERR_INVALID, "set_state: bad argument");
    IIV_HIP(hipDeviceSynchronize());
    uint8_t *base = reinterpret_cast<uint8_t *>(e->d_states + s0);
    const size_t pitch = sizeof(StreamState);
    if (what == IIV_STATE_RNG_PY || what == IIV_STATE_RNG_NP) {
        if (bytes != 625 * 4) return set_error(IIV_ERR_INVALID, "set_state: RNG state is 625 u32");
        for (int i = 0; i < n; i++) {
            uint32_t idx = ((const uint32_t *)buf)[(size_t)i * 625 + 624];
            if (idx > 624) return set_error(IIV_ERR_INVALID, "set_state: RNG index %u > 624 (stream %d)", idx, s0 + i);
        }
        const RngOffsets o = rng_offsets(what);
        IIV_HIP(hipMemcpy2D(base + o.mt, pitch, buf, 625 * 4, 624 * 4, (size_t)n, hipMemcpyHostToDevice));
        IIV_HIP(hipMemcpy2D(base + o.idx, pitch, (const uint8_t *)buf + 624 * 4, 625 * 4, 4, (size_t)n, hipMemcpyHostToDevice));
        return IIV_OK;
    }
    size_t off, want;
    bool writable;
    if (state_item(e->mode, what, off, want, writable) || !writable)
        return set_error(IIV_ERR_INVALID, "set_state: item %d is not settable", what);
    if (bytes != want) return set_error(IIV_ERR_INVALID, "set_state: item %d is %zu bytes, got %zu", what, want, bytes);
    if (what == IIV_STATE_UP_MAIN || what == IIV_STATE_UP_AUX)   // (compact_up_kernel rewrites BOTH banks' 16-bit copies from up[])
        if (int rc = materialise_up(e, s0, n)) return rc;
    IIV_HIP(hipMemcpy2D(base + off, pitch, buf, bytes, bytes, (size_t)n, hipMemcpyHostToDevice));
    if (what == IIV_STATE_UP_MAIN || what == IIV_STATE_UP_AUX) {
        if (int rc = launch(compact_up_kernel, "compact_up_kernel launch", dim3(n), dim3(256), 0, 0, e->d_states + s0)) return rc;
        return hip_check(hipDeviceSynchronize(), "compact_up sync");
    }
    return IIV_OK;
}

// The small items of ONE stream, enqueued on `st` behind the launches already there -- no device-wide synchronisation, no
// blocking copy: the bytes are taken into a pinned slot before the call returns.
int encoder_set_state_async(Encoder *e, int s, int what, const void *buf, size_t bytes, hipStream_t st)
{
    if (!e || !buf || s < 0 || s >= e->n_streams) return set_error(IIV_ERR_INVALID, "set_state_async: bad argument");
    if (what != IIV_STATE_OUT_OF_WORK && what != IIV_STATE_RNG_PY && what != IIV_STATE_RNG_NP)
        return set_error(IIV_ERR_INVALID, "set_state_async: item %d (only OUT_OF_WORK, RNG_PY, RNG_NP)", what);
    const size_t want = what == IIV_STATE_OUT_OF_WORK ? 8 : 625 * 4;
    if (bytes != want) return set_error(IIV_ERR_INVALID, "set_state_async: item %d is %zu bytes, got %zu", what, want, bytes);
    if (what != IIV_STATE_OUT_OF_WORK && ((const uint32_t *)buf)[624] > 624)
        return set_error(IIV_ERR_INVALID, "set_state_async: RNG index %u > 624", ((const uint32_t *)buf)[624]);
    if (!e->h_small) {
        HostBuf<uint8_t> ring;
        Event ev[kSmallSlots];
        if (int rc = ring.alloc(kSmallSlots * kSmallBytes, hipHostMallocDefault, "hipHostMalloc(state staging)")) return rc;
        for (int k = 0; k < kSmallSlots; k++)
            if (int rc = ev[k].create(hipEventDisableTiming, "event")) return rc;
        e->h_small = std::move(ring);
        for (int k = 0; k < kSmallSlots; k++) e->small_ev[k] = std::move(ev[k]);
        e->small_slot = -kSmallSlots;   // (the first round of the ring has nothing to wait for)
    }
    const int k = e->small_slot < 0 ? e->small_slot + kSmallSlots : e->small_slot;
    if (e->small_slot >= 0) IIV_HIP(hipEventSynchronize(e->small_ev[k]));   // the copies that last used this slot are done
    e->small_slot = e->small_slot < 0 ? e->small_slot + 1 : (e->small_slot + 1) % kSmallSlots;
    uint8_t *slot = e->h_small + (size_t)k * kSmallBytes;
    memcpy(slot, buf, bytes);
    uint8_t *base = reinterpret_cast<uint8_t *>(e->d_states + s);
    if (what == IIV_STATE_OUT_OF_WORK) {
        IIV_HIP(hipMemcpyAsync(base + offsetof(StreamState, out_of_work), slot, 8, hipMemcpyHostToDevice, st));
    } else {
        const RngOffsets o = rng_offsets(what);
        IIV_HIP(hipMemcpyAsync(base + o.mt, slot, 624 * 4, hipMemcpyHostToDevice, st));
        IIV_HIP(hipMemcpyAsync(base + o.idx, slot + 624 * 4, 4, hipMemcpyHostToDevice, st));
    }
    IIV_HIP(hipEventRecord(e->small_ev[k], st));
    return IIV_OK;
}

static_assert(offsetof(StreamState, up) == 2 * 8192 && offsetof(StreamState, mt_np) == offsetof(StreamState, mt_py) + 2496 &&
                  offsetof(StreamState, mt_py_idx) == offsetof(StreamState, mt_np) + 2496 &&
                  offsetof(StreamState, mt_np_idx) == offsetof(StreamState, mt_py_idx) + 4,
              "iiv_video_state is copied in blocks that follow StreamState's layout");

int encoder_get_video_state(Encoder *e, int s, iiv_video_state *out)
{
    if (!e || !out || s < 0 || s >= e->n_streams) return set_error(IIV_ERR_INVALID, "get_video_state: bad argument");
    uint8_t *base = reinterpret_cast<uint8_t *>(e->d_states + s);
    IIV_HIP(hipDeviceSynchronize());
    int rc = pack(e->mode, 1, base + offsetof(StreamState, mem[0]), base + offsetof(StreamState, mem[1]), e->d_packed, 0);
    if (!rc) rc = materialise_up(e, s, 1);
    if (rc) return rc;
    IIV_HIP(hipMemcpy(out->mem_main, base, 2 * 8192 + 2 * 8192 * 4, hipMemcpyDeviceToHost));   // mem[2] | up[2]
    uint32_t rng[1250];
    IIV_HIP(hipMemcpy(rng, base + offsetof(StreamState, mt_py), sizeof(rng), hipMemcpyDeviceToHost));
    memcpy(out->rng_py, rng, 2496);
    memcpy(out->rng_np, rng + 624, 2496);
    out->rng_py[624] = rng[1248];
    out->rng_np[624] = rng[1249];
    IIV_HIP(hipMemcpy(out->out_of_work, base + offsetof(StreamState, out_of_work), 8, hipMemcpyDeviceToHost));
    IIV_HIP(hipMemcpy(out->packed, e->d_packed, 4096 * 8, hipMemcpyDeviceToHost));
    return IIV_OK;
}

// iiv_video_brief of one stream, assembled on the device so that it travels in one copy: priority sums, hole bytes,
// out_of_work and both MT19937 states in the struct's own layout
__global__ __launch_bounds__(256) void brief_kernel(const StreamState *__restrict__ S, iiv_video_brief *__restrict__ out)
{
    __shared__ long long sums[2][4];
    __shared__ int holes[2][4];
    const int tid = threadIdx.x;
    long long a[2] = {0, 0};
    int h[2] = {0, 0};
    for (int b = 0; b < 2; b++)
        for (int i = tid; i < 8192; i += 256) {
            a[b] += up_value(*S, b, i);
            if (is_hole(i & 255) && S->mem[b][i] != 0) h[b]++;
        }
    for (int i = tid; i < 624; i += 256) {
        out->rng_py[i] = S->mt_py[i];
        out->rng_np[i] = S->mt_np[i];
    }
    for (int b = 0; b < 2; b++) {
        for (int d = 1; d < 64; d <<= 1) {
            a[b] += __shfl_xor(a[b], d, 64);
            h[b] += __shfl_xor(h[b], d, 64);
        }
        if ((tid & 63) == 0) {
            sums[b][tid >> 6] = a[b];
            holes[b][tid >> 6] = h[b];
        }
    }
    __syncthreads();
    if (tid < 2) {
        out->priority_sum[tid] = sums[tid][0] + sums[tid][1] + sums[tid][2] + sums[tid][3];
        out->hole_bytes[tid] = holes[tid][0] + holes[tid][1] + holes[tid][2] + holes[tid][3];
        out->out_of_work[tid] = S->out_of_work[tid];
        (tid ? out->rng_np : out->rng_py)[624] = tid ? S->mt_np_idx : S->mt_py_idx;
    }
}

int encoder_get_video_brief(Encoder *e, int s, iiv_video_brief *out)
{
    if (!e || !out || s < 0 || s >= e->n_streams) return set_error(IIV_ERR_INVALID, "get_video_brief: bad argument");
    IIV_HIP(hipDeviceSynchronize());
    if (int rc = launch(brief_kernel, "brief_kernel launch", dim3(1), dim3(256), 0, 0, e->d_states + s, e->d_brief)) return rc;
    IIV_HIP(hipMemcpy(out, e->d_brief, sizeof(iiv_video_brief), hipMemcpyDeviceToHost));
    return IIV_OK;
}

// The same, enqueued on `st` behind whatever was launched there: nothing waits.  host_out holds the brief once the
// stream has been synchronised (iiv_encoder_check does); pinned memory makes the copy truly asynchronous.
int encoder_get_video_brief_async(Encoder *e, int s, iiv_video_brief *out, hipStream_t st)
{
    if (!e || !out || s < 0 || s >= e->n_streams) return set_error(IIV_ERR_INVALID, "get_video_brief_async: bad argument");
    if (int rc = launch(brief_kernel, "brief_kernel launch", dim3(1), dim3(256), 0, st, e->d_states + s, e->d_brief)) return rc;
    IIV_HIP(hipMemcpyAsync(out, e->d_brief, sizeof(iiv_video_brief), hipMemcpyDeviceToHost, st));
    return IIV_OK;
}

int encoder_set_video_state(Encoder *e, int s, const iiv_video_state *in)
{
    if (!e || !in || s < 0 || s >= e->n_streams) return set_error(IIV_ERR_INVALID, "set_video_state: bad argument");
    if (in->rng_py[624] > 624 || in->rng_np[624] > 624) return set_error(IIV_ERR_INVALID, "set_video_state: RNG index > 624");
    uint8_t *base = reinterpret_cast<uint8_t *>(e->d_states + s);
    IIV_HIP(hipDeviceSynchronize());
    IIV_HIP(hipMemcpy(base, in->mem_main, 2 * 8192 + 2 * 8192 * 4, hipMemcpyHostToDevice));
    uint32_t rng[1250];
    memcpy(rng, in->rng_py, 2496);
    memcpy(rng + 624, in->rng_np, 2496);
    rng[1248] = in->rng_py[624];
    rng[1249] = in->rng_np[624];
    IIV_HIP(hipMemcpy(base + offsetof(StreamState, mt_py), rng, sizeof(rng), hipMemcpyHostToDevice));
    IIV_HIP(hipMemcpy(base + offsetof(StreamState, out_of_work), in->out_of_work, 8, hipMemcpyHostToDevice));
    // (both banks' priorities were just written)
    if (int rc = launch(compact_up_kernel, "compact_up_kernel launch", dim3(1), dim3(256), 0, 0, e->d_states + s)) return rc;
    return hip_check(hipDeviceSynchronize(), "compact_up sync");
}

int encoder_profile(Encoder *e, int enable)
{
    if (!e) return set_error(IIV_ERR_INVALID, "profile: null encoder");
    e->profiling = enable ? 1 : 0;
    if (enable) {
        e->ev_class.clear();
        e->ms[0] = e->ms[1] = 0;
        e->launches[0] = e->launches[1] = 0;
        e->form_launches[0] = e->form_launches[1] = e->form_launches[2] = e->form_launches[3] = 0;
    }
    return IIV_OK;
}

int encoder_launch_forms(Encoder *e, int64_t counts[4])
{
    if (!e || !counts) return set_error(IIV_ERR_INVALID, "launch_forms: bad argument");
    for (int k = 0; k < 4; k++) counts[k] = e->form_launches[k];
    return IIV_OK;
}

int encoder_input_stats(Encoder *e, double stats[2], int *form)
{
    if (!e) return set_error(IIV_ERR_INVALID, "input_stats: null encoder");
    if (stats) {
        stats[0] = e->tie_rate;
        stats[1] = e->ops_per_launch;
    }
    // (what a full-batch launch would run now, not what a round whose streams' banks differ ends up with)
    if (form) *form = shared_form_now(launch_inputs(*e)) ? IIV_GREEDY_WAVE_SHARED : IIV_GREEDY_WAVE_PLAIN;
    return IIV_OK;
}

int encoder_profile_read(Encoder *e, double ms[2], int64_t launches[2])
{
    if (!e) return set_error(IIV_ERR_INVALID, "profile_read: null encoder");
    for (size_t i = 0; i < e->ev_class.size(); i++) {   // the intervals recorded since the last read (iiv_encode.hip: prof_begin)
        IIV_HIP(hipEventSynchronize(e->ev_pool[2 * i + 1]));
        float t = 0;
        IIV_HIP(hipEventElapsedTime(&t, e->ev_pool[2 * i], e->ev_pool[2 * i + 1]));
        e->ms[e->ev_class[i]] += t;
        e->launches[e->ev_class[i]] += 1;
    }
    e->ev_class.clear();
    ms[0] = e->ms[0];
    ms[1] = e->ms[1];
    launches[0] = e->launches[0];
    launches[1] = e->launches[1];
    return IIV_OK;
}

__global__ void error_scan_kernel(const StreamState *states, int n, int *result)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && states[i].error) {
        atomicMin(&result[0], i);
    }
}

int encoder_check(Encoder *e, int *bad_stream, hipStream_t st)
{
    if (!e) return set_error(IIV_ERR_INVALID, "check: null encoder");
    int *d_res = e->d_result;
    int init = 0x7fffffff;
    int rc = hip_check(hipMemcpyAsync(d_res, &init, sizeof(int), hipMemcpyHostToDevice, st), "check init");
    if (!rc) {
        rc = launch(error_scan_kernel, "error_scan_kernel launch", dim3((e->n_streams + 255) / 256), dim3(256), 0, st, e->d_states, e->n_streams,
                    d_res);
    }
    int first = 0x7fffffff;
    if (!rc) rc = hip_check(hipMemcpyAsync(&first, d_res, sizeof(int), hipMemcpyDeviceToHost, st), "check read");
    if (!rc) rc = hip_check(hipStreamSynchronize(st), "check sync");
    if (rc) return rc;
    if (first == 0x7fffffff) return IIV_OK;
    if (bad_stream) *bad_stream = first;
    int32_t code = 0;
    IIV_HIP(hipMemcpy(&code, reinterpret_cast<uint8_t *>(e->d_states + first) + offsetof(StreamState, error), 4,
                      hipMemcpyDeviceToHost));
    static const char *names[] = {"",
                                  "memory map has non-zero screen-hole bytes (video.py:87)",
                                  "negative update_priority (video.py:117)",
                                  "DHGR content byte has the palette bit set (video.py:137)",
                                  "pushed-entry capacity exceeded",
                                  "next() on a stream with no generator",
                                  "internal: greedy loop guard tripped",
                                  "internal: prefix sort exhausted before the opcode budget",
                                  "internal: a stream's bank differs from its workgroup's shared table"};
    int is_overflow = code == kErrPushedOverflow;
    return set_error(is_overflow ? IIV_ERR_OVERFLOW : IIV_ERR_ASSERT, "stream %d: %s", first,
                     (code > 0 && code < 9) ? names[code] : "unknown error");
}

}  // namespace iiv

// ------------------------------------------------------------------------- C ABI
// (an iiv_encoder is the host object: the entry points forward to the functions above, which check their arguments)
extern "C" {

int iiv_encoder_create(int mode, const uint16_t *d_table, const uint16_t *d_store_table, const int32_t dm[256], int n_streams, iiv_encoder **out)
{
    return iiv::encoder_create(mode, d_table, d_store_table, dm, n_streams, out);
}
void iiv_encoder_destroy(iiv_encoder *enc) { delete enc; }
int iiv_encoder_snapshot(iiv_encoder *enc, void *stream) { return iiv::encoder_snapshot(enc, 0, (hipStream_t)stream); }
int iiv_encoder_rollback(iiv_encoder *enc, void *stream) { return iiv::encoder_rollback(enc, 0, (hipStream_t)stream); }
int iiv_encoder_snapshot_slot(iiv_encoder *enc, int slot, void *stream) { return iiv::encoder_snapshot(enc, slot, (hipStream_t)stream); }
int iiv_encoder_rollback_slot(iiv_encoder *enc, int slot, void *stream) { return iiv::encoder_rollback(enc, slot, (hipStream_t)stream); }
int iiv_encoder_set_option(iiv_encoder *enc, int option, int value) { return iiv::encoder_set_option(enc, option, value); }

int iiv_encoder_info(iiv_encoder *enc, int *mode, int *n_streams)
{
    if (!enc) return iiv::set_error(IIV_ERR_INVALID, "iiv_encoder_info: null encoder");
    if (mode) *mode = enc->mode;
    if (n_streams) *n_streams = enc->n_streams;
    return IIV_OK;
}

int iiv_encoder_get_state(iiv_encoder *enc, int stream_index, int what, void *host_buf, size_t bytes) { return iiv::encoder_get_state(enc, stream_index, what, host_buf, bytes); }
int iiv_encoder_set_state(iiv_encoder *enc, int stream_index, int what, const void *host_buf, size_t bytes) { return iiv::encoder_set_state(enc, stream_index, 1, what, host_buf, bytes); }
int iiv_encoder_set_state_range(iiv_encoder *enc, int first_stream, int n_streams, int what, const void *host_buf, size_t bytes_per_stream) { return iiv::encoder_set_state(enc, first_stream, n_streams, what, host_buf, bytes_per_stream); }
int iiv_encoder_set_state_async(iiv_encoder *enc, int stream_index, int what, const void *host_buf, size_t bytes, void *stream) { return iiv::encoder_set_state_async(enc, stream_index, what, host_buf, bytes, (hipStream_t)stream); }
int iiv_encoder_get_video_state(iiv_encoder *enc, int stream_index, iiv_video_state *host_out) { return iiv::encoder_get_video_state(enc, stream_index, host_out); }
int iiv_encoder_set_video_state(iiv_encoder *enc, int stream_index, const iiv_video_state *host_in) { return iiv::encoder_set_video_state(enc, stream_index, host_in); }
int iiv_encoder_get_video_brief(iiv_encoder *enc, int stream_index, iiv_video_brief *host_out) { return iiv::encoder_get_video_brief(enc, stream_index, host_out); }
int iiv_encoder_get_video_brief_async(iiv_encoder *enc, int stream_index, iiv_video_brief *host_out, void *stream) { return iiv::encoder_get_video_brief_async(enc, stream_index, host_out, (hipStream_t)stream); }

int iiv_encoder_render(iiv_encoder *enc, int first_stream, int n_streams, const uint8_t palette_rgb[48], uint8_t *d_rgb, void *stream)
{
    if (!enc || !palette_rgb || !d_rgb || first_stream < 0 || n_streams < 0 || n_streams > enc->n_streams - first_stream)
        return iiv::set_error(IIV_ERR_INVALID, "iiv_encoder_render: bad argument or stream range");
    if ((uintptr_t)d_rgb & 15) return iiv::set_error(IIV_ERR_INVALID, "iiv_encoder_render: d_rgb must be 16-byte aligned");
    if (n_streams == 0) return IIV_OK;
    // (the maps of a stream are the first 16 KiB of its StreamState, main then aux; the states lie sizeof(StreamState) apart)
    const uint8_t *base = reinterpret_cast<const uint8_t *>(enc->d_states + first_stream);
    return iiv::render_rgb(enc->mode, palette_rgb, n_streams, base + offsetof(iiv::StreamState, mem[0]),
                           base + offsetof(iiv::StreamState, mem[1]), sizeof(iiv::StreamState), d_rgb, (hipStream_t)stream);
}

int iiv_encoder_render_error(iiv_encoder *enc, int first_stream, int n_streams, const uint8_t palette_rgb[48], const uint8_t *d_ref,
                             int ref_width, uint64_t *d_out, void *stream)
{
    if (!enc || !palette_rgb || !d_ref || !d_out || first_stream < 0 || n_streams < 0 || n_streams > enc->n_streams - first_stream)
        return iiv::set_error(IIV_ERR_INVALID, "iiv_encoder_render_error: bad argument or stream range");
    if (ref_width != 280 && ref_width != 560)
        return iiv::set_error(IIV_ERR_INVALID, "iiv_encoder_render_error: ref_width must be 280 or 560");
    if (((uintptr_t)d_ref & 15) || ((uintptr_t)d_out & 7))
        return iiv::set_error(IIV_ERR_INVALID, "iiv_encoder_render_error: d_ref must be 16-byte aligned, d_out 8-byte aligned");
    if (n_streams == 0) return IIV_OK;
    const uint8_t *base = reinterpret_cast<const uint8_t *>(enc->d_states + first_stream);   // (as iiv_encoder_render)
    return iiv::render_error(enc->mode, palette_rgb, n_streams, base + offsetof(iiv::StreamState, mem[0]),
                             base + offsetof(iiv::StreamState, mem[1]), sizeof(iiv::StreamState), d_ref, ref_width, d_out,
                             (hipStream_t)stream);
}

int iiv_encoder_check(iiv_encoder *enc, int *bad_stream, void *stream) { return iiv::encoder_check(enc, bad_stream, (hipStream_t)stream); }
int iiv_encoder_profile(iiv_encoder *enc, int enable) { return iiv::encoder_profile(enc, enable); }
int iiv_encoder_profile_read(iiv_encoder *enc, double ms[2], int64_t launches[2]) { return iiv::encoder_profile_read(enc, ms, launches); }
int iiv_encoder_launch_forms(iiv_encoder *enc, int64_t counts[4]) { return iiv::encoder_launch_forms(enc, counts); }
int iiv_encoder_input_stats(iiv_encoder *enc, double stats[2], int *form) { return iiv::encoder_input_stats(enc, stats, form); }

int iiv_check_split_diff_table(int mode, const int32_t dm[256], const uint16_t *d_table, unsigned long long *mismatches,
                               void *stream)
{
    if ((mode != IIV_HGR && mode != IIV_DHGR) || !dm || !d_table || !mismatches)
        return iiv::set_error(IIV_ERR_INVALID, "iiv_check_split_diff_table: bad argument");
    return iiv::check_split_dw_table(mode, dm, d_table, mismatches, (hipStream_t)stream);
}

int iiv_check_diff_weight_pieces(int mode, const int32_t dm[256], const uint16_t *d_table, unsigned long long *mismatches,
                                 void *stream)
{
    if ((mode != IIV_HGR && mode != IIV_DHGR) || !dm || !d_table || !mismatches)
        return iiv::set_error(IIV_ERR_INVALID, "iiv_check_diff_weight_pieces: bad argument");
    return iiv::check_dw_piece_table(mode, dm, d_table, mismatches, (hipStream_t)stream);
}

int iiv_build_split_store_table(int mode, const int32_t dm[256], uint32_t *d_left, uint32_t *d_right,
                                uint16_t *d_expanded, void *stream)
{
    if (mode != IIV_HGR && mode != IIV_DHGR) return iiv::set_error(IIV_ERR_INVALID, "mode must be IIV_HGR or IIV_DHGR");
    if (!dm) return iiv::set_error(IIV_ERR_INVALID, "dm is NULL");
    return iiv::build_split_store_table(mode, dm, d_left, d_right, d_expanded, (hipStream_t)stream);
}

int iiv_build_narrow_store_table(int mode, const int32_t dm[256], const uint16_t *d_store_table, uint16_t *d_expanded,
                                 unsigned long long *n_mismatch, void *stream)
{
    if ((mode != IIV_HGR && mode != IIV_DHGR) || !dm || !d_store_table || !d_expanded || !n_mismatch)
        return iiv::set_error(IIV_ERR_INVALID, "iiv_build_narrow_store_table: bad argument");
    return iiv::build_narrow_store_table(mode, dm, d_store_table, d_expanded, n_mismatch, (hipStream_t)stream);
}

size_t iiv_split_table_entries(int mode, int right_half) { return iiv::split_entries(mode, right_half ? 1 : 0); }

}  // extern "C"
