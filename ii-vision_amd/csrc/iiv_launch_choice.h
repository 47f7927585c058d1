// iiv_launch_choice.h -- which greedy kernel a launch runs, and with what: the one place that decides it.  Plain host
// arithmetic on the encoder's options (no HIP type), so that a host compiler can build it alone
// (tests/test_launch_choice_host.py enumerates it).  iiv_encode.hip acts on the result; iiv_greedy.hip, iiv_team.hip and
// iiv_workgroup.hip launch what they are told.
#pragma once
#include <stdint.h>
#include "../../include/iivision.h"

namespace iiv {

constexpr int kSharedHgrMinStreams = 4096;   // 16 streams per workgroup x 256 CUs
constexpr int kSharedDhgrMinStreams = 2048;  // (at 1024 clips the LDS-shared form is 3 % behind the plain one)
// The LDS-shared form of the one-wave kernel keeps 16 waves per CU busy, the plain form 28.  On input whose steps are
// rarely decided by the nonces the shared form wins (DHGR +1-7 %, HGR +3-12 %); on picture-like input, where nearly every
// step takes the exact-nonce path with its extra wave reductions and LDS reads, 16 waves hide that latency worse than 28
// and it loses 5 %.  Both forms produce the same bytes, so the encoder picks by what its own kernels saw: they count the
// steps the nonces decided and the opcodes emitted, the counters come back with an asynchronous copy (never waited for:
// a call uses what an earlier call's copy has delivered), and a batch above this share runs the plain form.
// Round 6, re-measured per content (tools/content_kernel_split.py, greedy ms per 14336-stream launch, shared / plain):
//   DHGR  S-iid (share 0.03) 1.01 / 1.22   error-diffusion frames (0.14) 1.02 / 1.24   ordered-dither frames (0.36) 1.06 / 1.25
//         S-img (0.90) 1.30 / 1.30   -- two rounds of diets later the shared form is the better one up to ~85 %;
//   HGR   S-iid (0.02) 2.83 / 3.45   error-diffusion frames (0.11) 2.82 / 3.25   ordered-dither frames (0.36) 3.67 / 3.33
//         S-img (0.85) 6.26 / 3.37   -- its shared form keeps MT19937 in registers: the exact-nonce path is dear there.
constexpr unsigned kTieHeavyPercentDHGR = 85, kTieHeavyPercentHGR = 30;
// ... and so does a batch whose streams have little left to do per launch (converging content that is mostly out of work:
// a frame shown four times runs 5.7 M frames/s plain, 4.6 M shared -- the workgroups' table copy and stream queue are
// overhead that a launch of a few dozen real opcodes per stream does not repay)
constexpr unsigned kSharedMinOpsPerLaunch = 96;
constexpr int kTeamMaxStreams = 768;   // IIV_GREEDY_AUTO: at most this many streams run the team kernel
// Longest first (iiv_stream.h: GreedyArgs::perm): batches of at least this many streams run their one-wave launches in the
// order of what the streams' latest launches cost, re-sorted every kOrderEvery greedy launches (a stream's cost follows its
// content, which changes slowly; the sort is one 1024-thread workgroup, ~10 us)
constexpr int kOrderMinStreams = 2048;
constexpr int kOrderEvery = 4;

// what the decision reads of an encoder
struct LaunchInputs {
    int mode, n_streams;
    int greedy_mode, content_choice, fourth_offset, greedy_lds_pad, order_streams;   // the options (IIV_OPT_*)
    bool split;      // the split store table was built (dm given at creation)
    bool exact;      // ... and its narrow form reproduces the caller's store table (NarrowTables::exact)
    int tie_heavy;   // what the kernels' tie statistics said: -1 not known yet, 0 / 1 (tie_heavy_input)
};

enum GreedyKernel { kKernelPlain = 0, kKernelShared = 1, kKernelTeam = 2, kKernelWorkgroup = 3 };   // (Encoder::form_launches' indices)

struct LaunchChoice {
    GreedyKernel kernel;
    int joint;           // the workgroup kernel's `joint` argument (launch_greedy_workgroup), 0 elsewhere
    bool count_stats;    // the tie statistics decide something for this encoder: its one-wave launches count, its calls fetch them
    bool ordered;        // longest first: the one-wave kernel runs the streams in Encoder::d_perm's order and writes their costs
    int uniform_bank;    // GreedyArgs::uniform_bank
    bool zeroed_queue;   // the call resets the stream counters and its launches get one each (all but the team kernel's)
};

// does the batch fill the GPU with the LDS-shared form's workgroups?
inline bool fills_gpu(const LaunchInputs &in) { return in.n_streams >= (in.mode == IIV_HGR ? kSharedHgrMinStreams : kSharedDhgrMinStreams); }

// The one-wave kernel (split store table, pipelined loads) wins at every batch size: 28 streams resident per CU, and
// 1.16 us per opcode for a single stream against the 1.6 us of the 4-wave workgroup with its two barriers per opcode
// (tools/single_stream_probe.py); the workgroup kernel remains for encoders created without dm or whose narrow table is
// not exact, as a second implementation, and as the home of the joint content choice (with or without the fourth offset).
// With the reference's content byte the fourth offset runs in the one-wave and team kernels, whatever the kernel option says.
inline bool wave_kernels_run(const LaunchInputs &in) { return in.content_choice == IIV_CONTENT_TARGET && (in.fourth_offset || (in.split && in.exact && in.greedy_mode != IIV_GREEDY_WORKGROUP)); }

// Do this encoder's launches run the team kernel?  Few streams: a team of eight waves per stream scores the next entries
// of the list concurrently (iiv_team.hip); from ~900 streams on, one wave per stream fills the GPU.
inline bool team_kernel_runs(const LaunchInputs &in) { return wave_kernels_run(in) && (in.greedy_mode == IIV_GREEDY_TEAM || (in.greedy_mode == IIV_GREEDY_AUTO && in.n_streams <= kTeamMaxStreams)); }

// The form of the one-wave kernel a launch of a full batch would run now: the LDS-shared one on request; otherwise for
// batches that fill the GPU with its workgroups, unless the kernels have reported input on which the plain form is the
// faster one (until they have reported: HGR shared, DHGR plain -- the better guess for each).
inline bool shared_form_now(const LaunchInputs &in)
{
    return in.greedy_mode == IIV_GREEDY_WAVE_SHARED || (in.greedy_mode != IIV_GREEDY_WAVE_PLAIN && fills_gpu(in) && (in.tie_heavy < 0 ? in.mode == IIV_HGR : in.tie_heavy == 0));
}

// `tie_heavy` from an interval of the kernels' counters: is the plain form the better one for this input?
inline int tie_heavy_input(int mode, unsigned long long ties, unsigned long long ops, unsigned long long runs)
{
    const unsigned long long heavy = mode == IIV_DHGR ? kTieHeavyPercentDHGR : kTieHeavyPercentHGR;
    return ties * 100ull > heavy * ops || ops < kSharedMinOpsPerLaunch * runs;
}

// The launch of one round.  uniform_bank: 0 / 1 = every stream that emits opcodes in the round works on that bank, -1 = they differ.
inline LaunchChoice choose_launch(const LaunchInputs &in, int uniform_bank)
{
    // (the statistics matter only to a batch that fills the GPU with the one-wave kernel in its automatic form choice: a
    // single-clip Video, a forced form, the team and the workgroup kernel should not pay for counters, a reduction launch
    // and a copy per call)
    const bool stats = in.split && in.exact && (in.greedy_mode == IIV_GREEDY_AUTO || in.greedy_mode == IIV_GREEDY_WAVE) &&
                       in.content_choice == IIV_CONTENT_TARGET && fills_gpu(in);
    const bool team = team_kernel_runs(in);
    LaunchChoice c{kKernelWorkgroup, 0, stats, false, uniform_bank, !team};
    if (!wave_kernels_run(in)) {
        c.joint = in.content_choice == IIV_CONTENT_JOINT ? 2 : in.content_choice == IIV_CONTENT_JOINT_SPLIT ? 1 : 0;
    } else if (team) {
        c.kernel = kKernelTeam;
    } else {
        if (in.greedy_mode == IIV_GREEDY_WAVE_PLAIN) c.uniform_bank = -1;
        // (the shared form needs every stream of the round on one bank -- always so in HGR -- and all of the CU's LDS)
        c.kernel = shared_form_now(in) && c.uniform_bank >= 0 && in.greedy_lds_pad == 0 ? kKernelShared : kKernelPlain;
        c.ordered = in.n_streams >= kOrderMinStreams && in.order_streams != 0;
    }
    return c;
}

}  // namespace iiv
