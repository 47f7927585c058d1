// iiv_encoder.h -- the encoder's host object, shared by iiv_encoder.hip (creation, options, state, read-outs) and
// iiv_encode.hip (planning and launching).
#pragma once

#include "iiv_host.h"
#include "iiv_launch_choice.h"
#include "iiv_stream.h"
#include <vector>

namespace iiv {

struct GenState {
    int active;   // 0 = no generator, 1 = live on the device, 2 = created (lazily), prologue pending
    int is_aux, frame;
};

constexpr int kSmallSlots = 4;          // iiv_encoder_set_state_async's staging ring
constexpr size_t kSmallBytes = 2560;    // >= 625 words

// Every device buffer, pinned buffer and event is held by its owner (iiv_host.h), every plain field starts at the value
// written here: destroying the object releases everything.
struct Encoder {
    int mode = 0;
    int n_streams = 0;
    const uint16_t *d_table = nullptr;   // the caller's
    const uint16_t *d_store = nullptr;
    DeviceBuf<uint32_t> d_left, d_right;  // split store table (iiv_stream.h), built at creation when dm is given
    NarrowTables nt{};                    // the narrow form of the split store table the greedy kernels read (iiv_stream.h) ...
    DeviceBuf<uint8_t> nt_storage;        // ... and the allocation it points into
    DeviceBuf<uint32_t> d_dwl, d_dwr;     // split diff-weight table, likewise (IIV_DW_SPLIT; built on first use)
    DeviceBuf<uint32_t> d_left_t, d_right_t;  // split store table, content innermost (IIV_CONTENT_JOINT_SPLIT; built on first use)
    DeviceBuf<uint32_t> d_joint_l, d_joint_r; // narrow form, content innermost, two byte values per word (IIV_CONTENT_JOINT; built on first use)
    DeviceBuf<iiv_video_brief> d_brief;       // iiv_encoder_get_video_brief's staging struct
    DeviceBuf<ulonglong2> d_strings;  // colour string of every masked value (recurrence mode)
    DeviceBuf<uint32_t> d_hgr_dots;   // HGR: the window -> dots lookups the prologue copies into LDS (iiv_edit.h: hgr_dot_slot_lo)
    DeviceBuf<uint32_t> d_dw_pieces;  // the diff weights' pair-term table the prologue copies into LDS (iiv_tables.hip: dw_piece_kernel)
    DeviceBuf<uint16_t> d_sub;        // 16x16 substitute costs
    int dw_mode = IIV_DW_TABLE;       // IIV_DW_TABLE / IIV_DW_RECURRENCE (the default when dm is given)
    int greedy_mode = IIV_GREEDY_AUTO;   // IIV_GREEDY_WAVE / IIV_GREEDY_WORKGROUP / IIV_GREEDY_AUTO
    int partial_sort = 1;             // allow the prologue's prefix sort when the budget is known
    int greedy_lds_pad = 0;           // IIV_OPT_GREEDY_LDS_PAD
    int content_choice = IIV_CONTENT_TARGET;   // IIV_OPT_CONTENT_CHOICE
    int fourth_offset = 0;            // IIV_OPT_FOURTH_OFFSET
    DeviceBuf<StreamState> d_states;
    DeviceBuf<StreamState> d_snapshot[2];  // iiv_encoder_snapshot copies (lazily allocated; slot 1: iiv_encoder_snapshot_slot)
    // iiv_encoder_set_state_async: a small ring of pinned staging slots (one allocation), an event behind each slot's copies
    HostBuf<uint8_t> h_small;
    Event small_ev[kSmallSlots];
    int small_slot = 0;
    // live hand-over (iiv_encode_live): two opcode queues in coherent host memory (lazily allocated), and the one / the tag
    // the launches of the call in progress write to (NULL outside such a call)
    HostBuf<unsigned long long> h_live[2];
    unsigned long long *d_live[2] = {nullptr, nullptr}, *live_now = nullptr;   // (d_live: the same memory as the device addresses it)
    uint32_t live_tag = 0;
    // generator bookkeeping: one entry while every stream has run the same schedule, else one per stream
    std::vector<GenState> gens{GenState{0, 0, 0}}, snap_gens[2];
    // launch descriptors: pinned staging ring -> device buffer, both grown on demand
    HostBuf<LaunchSeg> h_segs[2];
    Event seg_ev[2];
    int seg_slot = 0;
    DeviceBuf<LaunchSeg> d_segs;
    DeviceBuf<int> d_queue;     // one stream counter per launch round of a call (persistent greedy workgroups), zeroed per call
    // what the one-wave kernels saw (iiv_launch_choice.h: tie_heavy_input): device counters, their pinned host copy, the event behind the copy
    DeviceBuf<unsigned long long> d_tie_stats;
    HostBuf<unsigned long long> h_tie_stats;
    unsigned long long tie_seen[3] = {0, 0, 0};
    Event tie_ev;
    bool tie_copy_pending = false;
    int tie_heavy = -1;         // -1: not known yet, 0 / 1
    double tie_rate = 0.0;      // of the latest interval looked at
    double ops_per_launch = 0.0;  // real (not padding) opcodes per stream and launch, likewise
    // scratch for encoder_check / IIV_STATE_PACKED
    DeviceBuf<int> d_result;
    DeviceBuf<uint64_t> d_packed;
    // profiling
    int profiling = 0;
    std::vector<Event> ev_pool;
    std::vector<int> ev_class;  // class of interval i = events [2i, 2i+1]
    double ms[2] = {0, 0};
    int64_t launches[2] = {0, 0};
    int64_t form_launches[4] = {0, 0, 0, 0};   // greedy launches since profiling was switched on: one-wave plain / LDS-shared, team, workgroup
    // longest-first launch order of the one-wave kernel: what every stream's latest launch cost, the permutation in use
    DeviceBuf<uint32_t> d_cost;
    DeviceBuf<int> d_perm;
    int order_countdown = 2;    // greedy launches until the next re-sort (the first launches have no history: two of them, then the first sort)
    int order_streams = 1;      // IIV_OPT_STREAM_ORDER: 1 (default) / 0
};

// what the launch decision reads of an encoder (iiv_launch_choice.h)
inline LaunchInputs launch_inputs(const Encoder &e)
{
    return LaunchInputs{e.mode, e.n_streams, e.greedy_mode, e.content_choice, e.fourth_offset, e.greedy_lds_pad, e.order_streams,
                        e.d_left != nullptr, e.nt.exact != 0, e.tie_heavy};
}

// iiv_encode.hip: perm = the streams by descending cost, or (identity != 0) perm[i] = i
int launch_order_streams(const uint32_t *d_cost, int n, int *d_perm, int identity, hipStream_t st);

}  // namespace iiv

// the C ABI's handle (include/iivision.h) is the host object itself
struct iiv_encoder : iiv::Encoder {};
