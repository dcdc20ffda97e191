// The IK-DDP launch plan: kernel, grid and workgroup size of every launch of a batch solve, as pure functions of the batch's sizes, the
// host's latest look at the active counter and one snapshot of the scheduling knobs.  Host code: no HIP call, no global.  run_ddp
// (bunmpc_ik_capi.hip) decides with it, ik_launch (ik_ddp.hip) executes it, bmpc_ik_plan_iteration exports it (tests/test_ik_plan_cpu.py).
#pragma once

namespace bunmpc {

// Problems whose line search goes past four step lengths are few and always the same ones (Go2 H = 60, 1024 problems: three
// problems cause a second round in 76 of the 100 iterations), and a second round costs the whole batch a rollout's latency.
// Such a problem is flagged (S_WIDE) and from then on gets all ten step lengths at once, on three workgroups.
constexpr int kWideMax = 32;
// The express lane (ik_select_kernel / ik_fused_kernel in ik_ddp.hip): at most this many problems leave the batch early, out of
// batches of at least kExpressMinBatch; the lane looks at the batch in front of iterations kExpressFirstIter .. kExpressLastIter
constexpr int kExpressMax = 256, kExpressMinBatch = 64, kExpressFirstIter = 2, kExpressLastIter = 12;
constexpr int kMaxFusedCol = 63;    // T + 1 <= 64 nodes: the fused kernel and the express lane keep per-node flags in LDS; longer horizons run the four lock-step kernels only
constexpr int kTailChunk = 3;       // iterations per host look once few problems are left (one per look while many iterate)

// Every scheduling value of ONE DDP loop, each with the default and the meaning its bmpc_ik_set_* call documents (include/bunmpc.h);
// none has an effect on results.  The process keeps one IkKnobs as its defaults; a loop takes a copy when it starts, with the batch's
// own bmpc_ik_sched_t applied, and reads nothing else.  Thresholds count active problems, 0 = never.
struct IkKnobs {
    int spec_below = 1024, spec_one_wave_above = 0, all_steps = 0;      // line search: side by side at most; that on ONE wave above; all ten step lengths at most
    int gains_wave_below = 512, calcdiff_one_wave_above = 1024;         // Riccati pass: a gains wave at most; derivative pass: one wave per node pair above (pairs)
    int express_cap = 96, fused_direct = 16, blocking_waits = 1, debug_inject = 0;      // (debug_inject: bmpc_ik_sched_t's, tests)
    double express_near = 1.0;
};

// IkBatchArgs::fwd_spec, how the forward pass (line search) maps problems to waves: four problems per wave, step lengths one after the
// other; four step lengths of one problem at once on a workgroup of one / two / three waves; all ten at once on three such workgroups
enum IkFwdMap : int { IK_FWD_FOUR_PER_WAVE = 0, IK_FWD_SPEC_ONE_WAVE = 1, IK_FWD_SPEC_TWO_WAVES = 2, IK_FWD_SPEC_THREE_WAVES = 3, IK_FWD_ALL_STEPS = 4 };
enum IkKernel : int { IK_STATE = 0, IK_CALCDIFF, IK_CALCDIFF1, IK_BACKWARD1, IK_BACKWARD2, IK_FORWARD1, IK_FORWARD2, IK_FORWARD3, IK_KERNELS };
constexpr const char *kIkKernelNames[IK_KERNELS] = {"ik_state_kernel", "ik_calcdiff_kernel", "ik_calcdiff1_kernel", "ik_backward_kernel<1>",
                                                    "ik_backward_kernel<2>", "ik_forward_kernel<1>", "ik_forward_kernel<2>", "ik_forward_kernel<3>"};
struct IkLaunch { IkKernel kernel; unsigned grid, block; };
struct IkBatchPlan {
    bool fused_direct;  unsigned fused_grid;        // the whole DDP of every problem in ONE launch of the fused kernel, no host look in between
    int express_cap;    unsigned express_grid;      // what the express lane may take of this batch (0: no lane)
};
inline IkBatchPlan plan_batch(int B, int T, int maxiter, bool has_list, const IkKnobs &k) {
    const int cap = has_list && B >= kExpressMinBatch && T <= kMaxFusedCol ? k.express_cap : 0;
    return IkBatchPlan{has_list && B <= k.fused_direct && maxiter > 0 && T <= kMaxFusedCol, (unsigned)B, cap, (unsigned)(cap < kExpressMax ? cap : kExpressMax)};
}
struct IkIterPlan {
    int chunk;                      // iterations to enqueue before the next look
    IkFwdMap fwd;  int bwd_waves, n_launch;         // IkBatchArgs::fwd_spec, ::bwd_waves, ::n_launch (the look: an upper bound of the active list's length)
    IkLaunch state, calcdiff, backward, forward;
};
// one host look: `active` problems still iterate (launches cover those on the active list, or all B without one)
inline IkIterPlan plan_iteration(int active, int B, int T, bool has_list, bool has_wide, const IkKnobs &k) {
    IkIterPlan p;
    p.chunk = active <= k.spec_below ? kTailChunk : 1;
    p.fwd = active <= k.all_steps ? IK_FWD_ALL_STEPS : active <= k.spec_below / 3 ? IK_FWD_SPEC_THREE_WAVES
          : active <= k.spec_below ? IK_FWD_SPEC_TWO_WAVES : IK_FWD_FOUR_PER_WAVE;
    if (p.fwd == IK_FWD_SPEC_TWO_WAVES && k.spec_one_wave_above > 0 && active > k.spec_one_wave_above) p.fwd = IK_FWD_SPEC_ONE_WAVE;
    p.bwd_waves = active <= k.gains_wave_below ? 2 : 1; p.n_launch = active;
    const long problems = has_list ? (active < B ? active : B) : B, nodes = problems * (T + 1), pairs = problems * ((T + 1 + 1) / 2);
    const unsigned n = (unsigned)problems, wide = has_wide ? 2 * kWideMax : 0;      // the flagged problems' two extra workgroups each
    p.state = IkLaunch{IK_STATE, 2u * (unsigned)((nodes + 63) / 64), 64};          // two workgroups per 64 nodes
    p.calcdiff = pairs > k.calcdiff_one_wave_above ? IkLaunch{IK_CALCDIFF1, (unsigned)((pairs + 1) / 2), 128}      // two nodes per pair: a wave per pair, two pairs
                                                   : IkLaunch{IK_CALCDIFF, (unsigned)pairs, 128};                  // per workgroup, or a workgroup of two waves per pair
    p.backward = p.bwd_waves == 2 ? IkLaunch{IK_BACKWARD2, n, 128} : IkLaunch{IK_BACKWARD1, n, 64};
    p.forward = p.fwd == IK_FWD_ALL_STEPS ? IkLaunch{IK_FORWARD3, 3 * n, 192} : p.fwd == IK_FWD_SPEC_THREE_WAVES ? IkLaunch{IK_FORWARD3, n + wide, 192}
              : p.fwd == IK_FWD_SPEC_TWO_WAVES ? IkLaunch{IK_FORWARD2, n + wide, 128} : p.fwd == IK_FWD_SPEC_ONE_WAVE ? IkLaunch{IK_FORWARD1, n, 64}
              : IkLaunch{IK_FORWARD1, (n + 3) / 4, 64};
    return p;
}

}  // namespace bunmpc
