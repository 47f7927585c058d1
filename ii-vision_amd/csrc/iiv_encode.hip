// iiv_encode.hip -- video.Video.encode_frame on gfx950: the encoder's launch planning, its launches and their C ABI
// (the object itself: iiv_encoder.h / iiv_encoder.hip; which kernel a launch runs: iiv_launch_choice.h;
// reference: transcoder/video.py:72-301, transcoder/screen.py:383-547, transcoder/movie.py:56-111).
//
// One workgroup (or wave) per independent video stream; all stream state lives in HBM (StreamState) between
// launches and in LDS / registers inside one.  A launch round = for every stream, optionally a new generator
// (iiv_prologue.hip: prologue_kernel) and then its next n_ops opcodes (iiv_greedy.hip / iiv_team.hip /
// iiv_workgroup.hip).
//
// How the reference's heap is restated (proved equivalent on the CPU by
// oracle/iiv_oracle.c:step_struct against the imported reference):
//   * initial heap entries (-priority, nonce, page, offset) all have negative
//     keys, re-queued entries have key 65536-p > 0 (np.uint16 negation wraps,
//     video.py:178) => initial entries pop first, in sorted order;
//   * a byte whose update_priority is 0 is never selected again inside one
//     generator (video.py:130,159 skip it), so lazy deletion is permanent and
//     validity only ever decays;
//   * _compute_error's heap (video.py:290-301) only matters up to the first two
//     entries whose priority is non-zero => top-2 of (delta, nonce, offset).
// RNG: both global MT19937 streams are advanced on the device exactly as
// random.getrandbits(8) (high byte) and np.random.randint(0,256,n) (low byte)
// advance them (video.py:178,265,291).
#include "iiv_encoder.h"

namespace iiv {

// perm = the streams by descending cost (a counting sort over 1024 cost classes between the batch's cheapest and dearest
// stream; the order inside a class is whatever the atomics give -- any permutation is correct, a better one is faster).
// identity != 0: perm[i] = i.
__global__ __launch_bounds__(1024) void order_streams_kernel(const uint32_t *__restrict__ cost, int n, int *__restrict__ perm, int identity)
{
    __shared__ uint32_t lo_s, hi_s;
    __shared__ uint32_t count[1024], start[1024];
    const int tid = threadIdx.x;
    if (identity) {
        for (int i = tid; i < n; i += 1024) perm[i] = i;
        return;
    }
    if (tid == 0) lo_s = 0xffffffffu, hi_s = 0u;
    count[tid] = 0;
    __syncthreads();
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (int i = tid; i < n; i += 1024) {
        const uint32_t c = cost[i];
        lo = c < lo ? c : lo;
        hi = c > hi ? c : hi;
    }
    atomicMin(&lo_s, lo);
    atomicMax(&hi_s, hi);
    __syncthreads();
    lo = lo_s, hi = hi_s;
    const unsigned long long span = (unsigned long long)(hi - lo) + 1ull;
    auto cls = [&](uint32_t c) -> int { return (int)(((unsigned long long)(hi - c) * 1024ull) / span); };   // 0 = the dearest
    for (int i = tid; i < n; i += 1024) atomicAdd(&count[cls(cost[i])], 1u);
    __syncthreads();
    // exclusive prefix sum over the 1024 classes (one per thread: a plain two-level scan)
    __shared__ uint32_t wave_tot[16];
    uint32_t v = count[tid], incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
        if ((tid & 63) >= d) incl += o;
    }
    if ((tid & 63) == 63) wave_tot[tid >> 6] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < (tid >> 6); w++) base += wave_tot[w];
    start[tid] = base + incl - v;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) perm[atomicAdd(&start[cls(cost[i])], 1u)] = i;
}
int launch_order_streams(const uint32_t *d_cost, int n, int *d_perm, int identity, hipStream_t st)
{
    return launch(order_streams_kernel, "order_streams_kernel launch", dim3(1), dim3(1024), 0, st, d_cost, n, d_perm, identity);
}

static int prof_begin(Encoder *e, int cls, hipStream_t st, size_t &slot)
{
    slot = e->ev_class.size();
    if (e->ev_pool.size() < 2 * (slot + 1)) {
        Event a, b;
        if (int rc = a.create(hipEventDefault, "hipEventCreate")) return rc;
        if (int rc = b.create(hipEventDefault, "hipEventCreate")) return rc;
        e->ev_pool.push_back(std::move(a));
        e->ev_pool.push_back(std::move(b));
    }
    e->ev_class.push_back(cls);
    IIV_HIP(hipEventRecord(e->ev_pool[2 * slot], st));
    return IIV_OK;
}

static int prof_end(Encoder *e, size_t slot, hipStream_t st) { return hip_check(hipEventRecord(e->ev_pool[2 * slot + 1], st), "hipEventRecord"); }

// One stream's segment list -> one LaunchSeg per round (a segment that emits nothing takes no
// round).  `rounds` receives the descriptors; gs is the stream's generator bookkeeping.
static int plan_stream(Encoder *e, int stream, const iiv_segment *segs, int n_segs, int n_frames, GenState &gs,
                       std::vector<LaunchSeg> &rounds, size_t &total_ops)
{
    rounds.clear();
    size_t done = 0;
    for (int i = 0; i < n_segs; i++) {
        const iiv_segment &g = segs[i];
        if (g.n_ops < 0 || g.frame < 0 || g.frame >= n_frames || (g.is_aux != 0 && g.is_aux != 1) ||
            (e->mode == kHGR && g.is_aux))
            return set_error(IIV_ERR_INVALID, "iiv_encode: bad segment %d (stream %d)", i, stream);
        if (g.n_ops == 0) {
            // encode_frame() only creates a lazy generator (video.py:72-93): remember
            // it, run nothing.  A later restart == 0 segment will start it.
            if (g.restart) gs = GenState{2, g.is_aux, g.frame};
            continue;
        }
        bool need_prologue = g.restart != 0;
        if (!g.restart) {
            if (!gs.active)
                return set_error(IIV_ERR_INVALID, "iiv_encode: segment %d continues no generator (stream %d)", i, stream);
            if (gs.is_aux != g.is_aux || gs.frame != g.frame)
                return set_error(IIV_ERR_INVALID, "iiv_encode: segment %d continues a different target/bank (stream %d)", i,
                                 stream);
            if (gs.active == 2) need_prologue = true;
        }
        int need = -1;
        if (need_prologue) {
            need = 0;
            if (e->partial_sort) {
                // opcodes this generator can be asked for = n_ops of this segment and of the
                // restart == 0 segments that follow it -- known only if another restart comes
                // later in this call (otherwise a later call might continue the generator)
                long budget = g.n_ops;
                bool closed = false;
                for (int k = i + 1; k < n_segs; k++) {
                    if (segs[k].restart) {
                        closed = true;
                        break;
                    }
                    budget += segs[k].n_ops;
                }
                // (a step consumes at most one primary and two -- with the fourth offset three -- secondaries resolved to zero)
                const long per_op = e->fourth_offset ? 4 : 3;
                if (closed && per_op * budget <= kSelNeedMax) need = (int)(per_op * budget);
            }
        }
        gs = GenState{1, g.is_aux, g.frame};
        rounds.push_back(LaunchSeg{g.frame, g.is_aux, g.n_ops, (int32_t)done, need});
        done += (size_t)g.n_ops;
    }
    total_ops = done;
    return IIV_OK;
}

// copy n descriptors to the device through the pinned staging ring (truly asynchronous)
static int upload_segs(Encoder *e, const std::vector<LaunchSeg> &host, hipStream_t st)
{
    const size_t n = host.size();
    if (n > e->d_segs.count()) {
        IIV_HIP(hipStreamSynchronize(st));  // kernels of earlier calls may still read the old buffer
        if (int rc = e->d_segs.alloc(2 * n, "hipMalloc(launch descriptors)")) return rc;
    }
    const int k = e->seg_slot;
    e->seg_slot ^= 1;
    if (e->h_segs[k].count()) IIV_HIP(hipEventSynchronize(e->seg_ev[k]));  // the copy that last used this slot is done
    if (n > e->h_segs[k].count())
        if (int rc = e->h_segs[k].alloc(2 * n, hipHostMallocDefault, "hipHostMalloc(launch descriptors)")) return rc;
    memcpy(e->h_segs[k], host.data(), n * sizeof(LaunchSeg));
    IIV_HIP(hipMemcpyAsync(e->d_segs, e->h_segs[k], n * sizeof(LaunchSeg), hipMemcpyHostToDevice, st));
    IIV_HIP(hipEventRecord(e->seg_ev[k], st));
    return IIV_OK;
}

// zeroed stream counters for the n_rounds launches of a call, where its launches take any
static int reset_queues(Encoder *e, size_t n_rounds, hipStream_t st)
{
    if (!choose_launch(launch_inputs(*e), -1).zeroed_queue) return IIV_OK;
    if (n_rounds > e->d_queue.count()) {
        IIV_HIP(hipStreamSynchronize(st));  // kernels of earlier calls may still count in the old buffer
        if (int rc = e->d_queue.alloc(n_rounds * 2, "hipMalloc(stream counters)")) return rc;
    }
    IIV_HIP(hipMemsetAsync(e->d_queue, 0, n_rounds * sizeof(int), st));
    return IIV_OK;
}

// the streams' stat_* totals summed (one small launch per iiv_encode call, in front of the copy)
__global__ void tie_stats_kernel(const StreamState *states, int n, unsigned long long *out)
{
    unsigned long long a = 0, b = 0, c = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        a += states[i].stat_exact;
        b += states[i].stat_ops;
        c += states[i].stat_runs;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_xor(a, d, 64);
        b += __shfl_xor(b, d, 64);
        c += __shfl_xor(c, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[0], a);
        atomicAdd(&out[1], b);
        atomicAdd(&out[2], c);
    }
}

// tie statistics (iiv_launch_choice.h: tie_heavy_input): take in what an earlier call's copy has delivered, if it has
static void tie_stats_poll(Encoder *e)
{
    if (!e->tie_copy_pending || hipEventQuery(e->tie_ev) != hipSuccess) return;
    e->tie_copy_pending = false;
    if (e->h_tie_stats[2] < e->tie_seen[2] || e->h_tie_stats[1] < e->tie_seen[1] || e->h_tie_stats[0] < e->tie_seen[0]) {
        for (int k = 0; k < 3; k++) e->tie_seen[k] = e->h_tie_stats[k];   // (a rollback took the streams' totals back)
        return;
    }
    const unsigned long long ties = e->h_tie_stats[0] - e->tie_seen[0], ops = e->h_tie_stats[1] - e->tie_seen[1],
                             runs = e->h_tie_stats[2] - e->tie_seen[2];
    if (runs < 2ull * (unsigned long long)e->n_streams) return;   // (too little to judge by: keep counting)
    for (int k = 0; k < 3; k++) e->tie_seen[k] = e->h_tie_stats[k];
    e->tie_rate = ops ? (double)ties / (double)ops : 0.0;
    e->ops_per_launch = (double)ops / (double)runs;
    e->tie_heavy = tie_heavy_input(e->mode, ties, ops, runs);
}

// ... and ask for the counters as this call leaves them (asynchronous; one copy in flight at a time)
static int tie_stats_request(Encoder *e, hipStream_t st)
{
    if (!e->d_tie_stats || e->tie_copy_pending || !choose_launch(launch_inputs(*e), -1).count_stats) return IIV_OK;
    IIV_HIP(hipMemsetAsync(e->d_tie_stats, 0, 3 * sizeof(unsigned long long), st));
    const int blocks = e->n_streams < 64 * 256 ? (e->n_streams + 255) / 256 : 64;
    if (int rc = launch(tie_stats_kernel, "tie_stats_kernel launch", dim3(blocks), dim3(256), 0, st, e->d_states, e->n_streams, e->d_tie_stats))
        return rc;
    IIV_HIP(hipMemcpyAsync(e->h_tie_stats, e->d_tie_stats, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    IIV_HIP(hipEventRecord(e->tie_ev, st));
    e->tie_copy_pending = true;
    return IIV_OK;
}

// launch round r of a call: descriptors at d_round, stream i reads entry i * seg_stride; which greedy kernel and with
// what: choose_launch (iiv_launch_choice.h)
static int launch_round(Encoder *e, const uint8_t *d_main, const uint8_t *d_aux, int n_frames, size_t r, const LaunchSeg *d_round,
                        int seg_stride, bool any_prologue, int uniform_bank, uint8_t *d_ops, size_t ops_stride, hipStream_t st)
{
    size_t slot = 0;
    if (any_prologue) {
        if (e->profiling) { int prc = prof_begin(e, 0, st, slot); if (prc) return prc; }
        const PrologueArgs pa{e->d_states, d_main, d_aux, n_frames, e->n_streams, d_round, seg_stride, e->d_table, e->d_strings,
                              e->d_sub, e->d_dwl, e->d_dwr, e->d_hgr_dots, e->d_dw_pieces};
        if (int prc = launch_prologue(e->mode, e->dw_mode, pa, st)) return prc;
        if (e->profiling) { int prc = prof_end(e, slot, st); if (prc) return prc; }
    }
    const LaunchChoice c = choose_launch(launch_inputs(*e), uniform_bank);
    if (e->live_now && c.kernel != kKernelTeam)
        return set_error(IIV_ERR_INVALID, "iiv_encode_live: this encoder's launches do not run the team kernel");
    if (e->profiling) { int prc = prof_begin(e, 1, st, slot); if (prc) return prc; }
    int rc = IIV_OK;
    if (c.kernel == kKernelWorkgroup) {
        const bool packed = c.joint == 2;
        const WorkgroupArgs wa{e->d_states, d_main, d_aux, n_frames, e->n_streams, d_round, seg_stride, e->d_store,
                               packed ? e->d_joint_l : e->d_left_t, packed ? e->d_joint_r : e->d_right_t, d_ops, ops_stride};
        rc = launch_greedy_workgroup(e->mode, c.joint, e->fourth_offset != 0, wa, st);
    } else {
        // longest first: every kOrderEvery launches the streams are sorted by what their latest launch cost them (d_perm holds
        // the identity until the first sort)
        if (c.ordered && --e->order_countdown <= 0) {
            if (int rc = launch_order_streams(e->d_cost, e->n_streams, e->d_perm, 0, st)) return rc;
            e->order_countdown = kOrderEvery;
        }
        GreedyArgs a{e->d_states, d_main, d_aux, n_frames, e->n_streams, d_round, seg_stride, e->d_left, e->d_right, e->nt, d_ops,
                     ops_stride, e->greedy_lds_pad, c.uniform_bank, c.kernel == kKernelShared,
                     c.zeroed_queue ? e->d_queue + r : (int *)nullptr, e->fourth_offset != 0, c.count_stats,
                     c.ordered ? e->d_perm : (const int *)nullptr, c.ordered ? e->d_cost : (uint32_t *)nullptr};
        if (e->live_now) a.live = e->live_now, a.live_tag = e->live_tag;
        rc = c.kernel == kKernelTeam ? launch_greedy_team(e->mode, a, st) : launch_greedy_wave(e->mode, a, st);
    }
    if (rc || !e->profiling) return rc;
    e->form_launches[c.kernel]++;
    return prof_end(e, slot, st);
}

// every stream runs the same segment list
int encode(Encoder *e, const uint8_t *d_main, const uint8_t *d_aux, int n_frames, const iiv_segment *segs, int n_segs,
           uint8_t *d_ops, hipStream_t st)
{
    if (!e || !d_main || !segs || n_segs < 0 || n_frames <= 0 || (!d_ops && n_segs > 0))
        return set_error(IIV_ERR_INVALID, "iiv_encode: bad argument");
    if (e->mode == kDHGR && !d_aux) return set_error(IIV_ERR_INVALID, "iiv_encode: DHGR needs aux frames");
    if (e->gens.size() != 1)
        return set_error(IIV_ERR_INVALID, "iiv_encode: the streams have run different schedules (iiv_encode_streams); "
                                          "keep using iiv_encode_streams");
    GenState gs = e->gens[0];
    std::vector<LaunchSeg> rounds;
    size_t total = 0;
    if (int rc = plan_stream(e, 0, segs, n_segs, n_frames, gs, rounds, total)) return rc;
    e->gens[0] = gs;
    if (rounds.empty()) return IIV_OK;
    if (int rc = upload_segs(e, rounds, st)) return rc;
    // (the stream counters are the LDS-shared form's: the team kernel's launches -- few streams, the drop-in Video's path,
    // where a 4 us memset in front of every generator is felt -- do without)
    if (int rc = reset_queues(e, rounds.size(), st)) return rc;
    tie_stats_poll(e);
    for (size_t r = 0; r < rounds.size(); r++)
        if (int rc = launch_round(e, d_main, d_aux, n_frames, r, e->d_segs + r, 0, rounds[r].need >= 0, rounds[r].is_aux, d_ops, total * 6, st))
            return rc;
    return tie_stats_request(e, st);
}

// ---- live hand-over (include/iivision.h: iiv_encode_live)
constexpr int kLiveCap = 4096;   // opcodes per queue: what one call may emit

int encoder_live_queue(Encoder *e, int slot, uint64_t **host_queue, int *capacity)
{
    if (!e || slot < 0 || slot > 1 || !host_queue || !capacity) return set_error(IIV_ERR_INVALID, "live_queue: bad argument");
    if (e->n_streams != 1) return set_error(IIV_ERR_INVALID, "live_queue: a one-stream encoder's (this one has %d)", e->n_streams);
    if (!e->h_live[slot]) {
        // coherent (fine-grained) and mapped: a kernel's store is a write into host memory, seen by the host without any
        // synchronisation call
        HostBuf<unsigned long long> q;
        if (int rc = q.alloc(kLiveCap, hipHostMallocCoherent | hipHostMallocMapped, "hipHostMalloc(live queue)")) return rc;
        memset(q, 0, (size_t)kLiveCap * 8);   // (tag 0 is never used)
        void *dev = nullptr;
        IIV_HIP(hipHostGetDevicePointer(&dev, q, 0));
        e->h_live[slot] = std::move(q);
        e->d_live[slot] = static_cast<unsigned long long *>(dev);
    }
    *host_queue = reinterpret_cast<uint64_t *>(e->h_live[slot].get());
    *capacity = kLiveCap;
    return IIV_OK;
}

int encode_live(Encoder *e, const uint8_t *d_main, const uint8_t *d_aux, int n_frames, const iiv_segment *segs, int n_segs,
                uint8_t *d_ops, int slot, uint32_t tag, hipStream_t st)
{
    if (!e || slot < 0 || slot > 1 || !segs) return set_error(IIV_ERR_INVALID, "iiv_encode_live: bad argument");
    if (!e->h_live[slot]) return set_error(IIV_ERR_INVALID, "iiv_encode_live: no queue in that slot (iiv_encoder_live_queue)");
    if (tag == 0 || tag > 0xffffu) return set_error(IIV_ERR_INVALID, "iiv_encode_live: the tag must be 1 .. 65535");
    if (!team_kernel_runs(launch_inputs(*e)))   // (refused before anything is launched: the caller falls back to iiv_encode)
        return set_error(IIV_ERR_INVALID, "iiv_encode_live: this encoder's launches do not run the team kernel (options)");
    long long total = 0;
    for (int i = 0; i < n_segs; i++) total += segs[i].n_ops > 0 ? segs[i].n_ops : 0;
    if (total > kLiveCap) return set_error(IIV_ERR_INVALID, "iiv_encode_live: %lld opcodes, the queue holds %d", total, kLiveCap);
    e->live_now = e->d_live[slot];
    e->live_tag = tag;
    const int rc = encode(e, d_main, d_aux, n_frames, segs, n_segs, d_ops, st);
    e->live_now = nullptr;
    return rc;
}

// stream s runs segs[seg_begin[s] .. seg_begin[s + 1])
int encode_streams(Encoder *e, const uint8_t *d_main, const uint8_t *d_aux, int n_frames, const iiv_segment *segs,
                   const int32_t *seg_begin, uint8_t *d_ops, size_t ops_stride, hipStream_t st)
{
    if (!e || !d_main || !segs || !seg_begin || n_frames <= 0 || !d_ops)
        return set_error(IIV_ERR_INVALID, "iiv_encode_streams: bad argument");
    if (e->mode == kDHGR && !d_aux) return set_error(IIV_ERR_INVALID, "iiv_encode_streams: DHGR needs aux frames");
    const int S = e->n_streams;
    std::vector<GenState> gens = e->gens;
    if (gens.size() == 1) gens.assign((size_t)S, e->gens[0]);
    std::vector<std::vector<LaunchSeg>> plan((size_t)S);
    size_t n_rounds = 0;
    for (int s = 0; s < S; s++) {
        if (seg_begin[s + 1] < seg_begin[s]) return set_error(IIV_ERR_INVALID, "iiv_encode_streams: seg_begin must ascend");
        size_t total = 0;
        int rc = plan_stream(e, s, segs + seg_begin[s], seg_begin[s + 1] - seg_begin[s], n_frames, gens[(size_t)s],
                             plan[(size_t)s], total);
        if (rc) return rc;
        if (total * 6 > ops_stride)
            return set_error(IIV_ERR_INVALID, "iiv_encode_streams: stream %d emits %zu opcodes, ops_stride holds %zu", s,
                             total, ops_stride / 6);
        n_rounds = plan[(size_t)s].size() > n_rounds ? plan[(size_t)s].size() : n_rounds;
    }
    e->gens = gens;
    if (n_rounds == 0) return IIV_OK;
    std::vector<LaunchSeg> table(n_rounds * (size_t)S, LaunchSeg{0, 0, 0, 0, -1});
    std::vector<char> any_pro(n_rounds, 0);
    std::vector<int> bank(n_rounds, -2);   // -2: no stream emits in this round yet; -1: the streams' banks differ
    for (int s = 0; s < S; s++)
        for (size_t r = 0; r < plan[(size_t)s].size(); r++) {
            const LaunchSeg &g = plan[(size_t)s][r];
            table[r * (size_t)S + (size_t)s] = g;
            if (g.need >= 0) any_pro[r] = 1;
            if (g.n_ops > 0) bank[r] = bank[r] == -2 ? g.is_aux : (bank[r] == g.is_aux ? bank[r] : -1);
        }
    if (int rc = upload_segs(e, table, st)) return rc;
    if (int rc = reset_queues(e, n_rounds, st)) return rc;
    tie_stats_poll(e);
    for (size_t r = 0; r < n_rounds; r++)
        if (int rc = launch_round(e, d_main, d_aux, n_frames, r, e->d_segs + r * (size_t)S, 1, any_pro[r] != 0, bank[r] < 0 ? -1 : bank[r], d_ops, ops_stride, st))
            return rc;
    return tie_stats_request(e, st);
}

}  // namespace iiv

extern "C" {   // (the C ABI of the above, as in iiv_encoder.hip)

int iiv_encode(iiv_encoder *enc, const uint8_t *d_frames_main, const uint8_t *d_frames_aux, int n_frames,
               const iiv_segment *segments, int n_segments, uint8_t *d_ops_out, void *stream)
{
    return iiv::encode(enc, d_frames_main, d_frames_aux, n_frames, segments, n_segments, d_ops_out, (hipStream_t)stream);
}

int iiv_encoder_live_queue(iiv_encoder *enc, int slot, uint64_t **host_queue, int *capacity) { return iiv::encoder_live_queue(enc, slot, host_queue, capacity); }

int iiv_encode_live(iiv_encoder *enc, const uint8_t *d_frames_main, const uint8_t *d_frames_aux, int n_frames,
                    const iiv_segment *segments, int n_segments, uint8_t *d_ops_out, int slot, uint32_t tag, void *stream)
{
    return iiv::encode_live(enc, d_frames_main, d_frames_aux, n_frames, segments, n_segments, d_ops_out, slot, tag, (hipStream_t)stream);
}

int iiv_encode_streams(iiv_encoder *enc, const uint8_t *d_frames_main, const uint8_t *d_frames_aux, int n_frames,
                       const iiv_segment *segments, const int32_t *seg_begin, uint8_t *d_ops_out, size_t ops_stride,
                       void *stream)
{
    return iiv::encode_streams(enc, d_frames_main, d_frames_aux, n_frames, segments, seg_begin, d_ops_out, ops_stride, (hipStream_t)stream);
}

}  // extern "C"
