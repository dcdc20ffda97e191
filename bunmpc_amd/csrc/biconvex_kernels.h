// Internal (not part of the C-ABI): argument block shared by the host launcher
// (bunmpc_capi.hip) and the batched centroidal ADMM kernel (biconvex_admm.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <tuple>
#include <type_traits>

namespace bunmpc {

// Solver constants (reference defaults: biconvex.hpp:146-160, fista.hpp:52-60).
struct SolverConsts {
    double m;         // robot mass
    double rho;       // ADMM penalty
    double mu;        // friction coefficient of the "SoC" projection
    double beta;      // backtracking growth
    double tol;       // FISTA exit: ||y+ - y|| < tol
    double exit_tol;  // ADMM exit: ||A_f X - b_f|| < exit_tol
    int maxit;        // FISTA iteration cap
    int num_iters;    // ADMM iteration cap
};

// One batch of B independent BiConvexMP::optimize calls.  All pointers are DEVICE
// pointers.  Layout (row-major, batch outermost, then knot, then component):
//   cnt_plan [B][H][E][4]   rows [flag, x, y, z]            (set_contact_plan)
//   dt       [B][H]
//   x_init   [B][9]
// cost / bound description, one of two forms:
//   harness form (raw == 0): what create_cost_X / create_cost_F /
//     create_bound_constraints receive; the kernel applies those formulas itself.
//       W_X [.][9H], W_X_ter [.][9], W_F [.][3EH], bounds [.][H][6]  (batch stride 0 = shared)
//       X_nom [B][9H], X_ter [B][9]
//   raw form (raw == 1): what set_cost_x / set_cost_f / set_bounds_x leave behind
//       Qx, qx, lbx, ubx [B][9(H+1)] (Qx = diagonal), Qf [B][3EH], qf [B][3EH] or null
// state, in = warm start (set_warm_start_vars), out = last iterates:
//   X [B][9(H+1)], F [B][3EH], P [B][9(H+1)], L_x [B], L_f [B]
// telemetry: dyn_viol [B] (last ||A_f X - b_f||), hist [B][num_iters] or null,
//   stats [B][6] = {admm iters, sum F-FISTA iters, sum X-FISTA iters, F retries,
//                   X retries, status (0 ok, 2 NaN)}
struct BatchArgs {
    int B, H, raw, cold_start;
    int precision;   // 0: fp64 arithmetic; 1: fp32 iterates with fp64 decisions (harness form only)
    int exact_step_decisions;   // (set by the launcher; tests) 0: the headline kernel screens its certified loops lane by lane, then fp32 decisions; 1: every decision
                                // from the fp64 sums, no screen; 2: fp32 decisions without the screen (kernels without the screen read non-zero as 1)
    int certified_steps;        // (set by the launcher) fp64 batch kernels skip the backtracking test in phases whose step is certified: 1 force and
                                // motion phases, 2 force phases only, 0 none
    int force_foot_pairs;       // (set by the launcher; the eighth int: it sits where the block had padding, no other member moves) non-zero: the loop-constants
                                // build runs an eligible certified force phase two feet per lane (biconvex_admm_body.h: "two feet per lane"); read by no other kernel
    double L0_x, L0_f;
    SolverConsts c;
    const double *cnt_plan, *dt, *x_init;
    const double *W_X, *W_X_ter, *W_F, *bounds, *X_nom, *X_ter;
    long sW_X, sW_X_ter, sW_F, sbounds;
    const double *Qx, *qx, *lbx, *ubx, *Qf, *qf;
    double *X, *F, *P, *L_x, *L_f;
    double *dyn_viol, *hist;
    int *stats;
    int *trace;      // [B][num_iters][4] running totals {it_f, it_x, bt_f, bt_x} after every ADMM iteration, or null
    const double *cmtab;   // (set by the launcher) FISTA's momentum coefficients (t_k - 1) / t_{k+1}, k = 0 .. kMaxFistaIters - 1: a function of k alone
    // One slot for two pointers that never meet (the kernels' argument block keeps its size): the work-stealing kernel has its counter
    // here and records no certificate telemetry; every other launch has the caller's telemetry array or null.
    union {
        int *queue;          // (set by the launcher) the work-stealing kernel's device counter: problems handed out beyond the first per segment
        int *cert_phases;    // [B][2] {force phases, motion phases} that ran the certified loop from their first iteration, or null; written
                             // by the benchmark's instantiation alone (biconvex_admm_body.h: BAND), left as it is by every other kernel
    };
#ifdef BMPC_SIMD_STAMPS      // (the diagnostic build of tools/simd_mates_stamps.py alone; the shipped library has no such member and executes no stamp)
    unsigned long long *simd_stamps;      // (set by the launcher) [waves][8] or null: see simd_stamp, biconvex_admm_body.h
#endif
};

// Per-knot block-diagonal costs (bmpc_block_cost_t): the knot's symmetric block in place of its diagonal weights, raw form, fp64, one
// knot per lane (biconvex_admm_body.h: BQ).  Row-major full blocks; a side whose pointer is null takes BatchArgs' diagonal (Qx / Qf), which
// the kernel spreads into a block with exact zeros beside it.  Strides in doubles, 0 = one set of blocks shared by the batch.
struct BlockArgs {
    const double *Qx_blk;   // [.][H + 1][9][9]
    const double *Qf_blk;   // [.][H][3E][3E]
    long sQx_blk, sQf_blk;
};

// Costs that couple neighbouring knots (bmpc_band_cost_t): Q[(t, i), (t + 1, i)] = Q[(t + 1, i), (t, i)] = off[t][i] beside BatchArgs'
// diagonal (Qx / Qf) -- force-rate and momentum-rate terms.  Raw form, fp64, one knot per lane (biconvex_admm_body.h: KQ).  A side whose
// pointer is null has no coupling.  Strides in doubles, 0 = one set of weights shared by the batch.
struct BandArgs {
    const double *Qx_off;   // [.][H][9]
    const double *Qf_off;   // [.][H - 1][3E]
    long sQx_off, sQf_off;
};

// The Euclidean projection onto the friction cone (bmpc_cone_t, projection 1): per-foot friction coefficients, diagonal costs in either
// form, fp64, one knot per lane (biconvex_admm_body.h: CONE).  A null pointer: every foot has SolverConsts::mu.  Stride in doubles,
// 0 = one set of coefficients shared by the batch.
struct ConeArgs {
    const double *mu;       // [.][H][E]
    long smu;
};

// ... about per-contact surface normals (bmpc_contact_frame_t): ConeArgs and one unit normal, world frame, per problem, knot and foot --
// the cone's axis in place of world z (biconvex_admm_body.h: FRAME).  A layout of its own beside ConeArgs: the cone kernels' argument
// block stays what it is.  Stride in doubles, 0 = one set of normals shared by the batch.
struct ConeFrameArgs {
    const double *mu;       // [.][H][E], or null
    long smu;
    const double *normals;  // [.][H][E][3], never null
    long snormals;
};

constexpr int kStats = 6;
// LDS elements per knot of a problem (biconvex_admm_body.h: X 9, P 9, F 3E, R 9): 39 for four feet, 33 for two -- odd strides, so no
// two lanes of a segment share a bank (an odd E would make it even: only E = 2 and 4 are built)
constexpr int knot_lds(int E) { return 27 + 3 * E; }
constexpr int kSegLds = 15;            // ... and per problem in front of its knots (the x_init rows' multipliers, 9; XLDS: step constants, violation, counters)
constexpr int kLdsZeros = 54;          // zeros in LDS in front of all that (lanes without a knot read them)
constexpr int kMaxFistaIters = 4096;  // length of the momentum table (one per device, momentum_table below; the one-problem-per-wave kernel keeps its own in LDS: 32 KB + <= 30 KB of iterates < 64 KB)
constexpr int kMaxKnots = 256; // H + 1 <= 256: one knot per lane, one problem per <= 64 lanes of a wave, or (65 .. 256 knots) per workgroup of 2 / 4 waves

// Which Q a batch has beside BatchArgs' diagonal (Qx / Qf), and that Q's arrays: BlockArgs' for kBlocks, BandArgs' for kBand, x = the
// motion side (Qx_blk / Qx_off), f = the force side.  kCone: diagonal costs under the Euclidean cone projection -- a kernel family of
// its own like the two others, chosen the same way; f = ConeArgs' coefficients (null: the scalar), sf their stride, x unused.
// kConeFrame (internal: the exported plan_launch call knows the first three only): kCone about per-contact normals, a third family
// chosen exactly as kCone; f / sf as there, x = ConeFrameArgs' normals (never null), sx their stride
enum CostShape { kDiag = 0, kBlocks = 1, kBand = 2, kCone = 3, kConeFrame = 4 };
struct CostArgs {
    CostShape shape = kDiag;
    const double *x = nullptr, *f = nullptr;
    long sx = 0, sf = 0;
};
// What the kernels of each cost shape are built for, one row per CostShape in the enum's order -- stated here and nowhere else: the
// kernels' static_asserts (biconvex_admm_body.h: AdmmCfg), the launches' guards (biconvex_admm_inst.h: launch_shape), plan_launch and
// the C-ABI's refusals (bunmpc_capi.hip: check_cost) all read this table.
struct ShapeInfo {
    const char *kernel;     // the kernel template's name as plan_launch reports it (kDiag: of the fp64 batch kernel; plan_launch names its siblings)
    bool raw_only;          // the raw form only
    bool fp64_only;         // precision 0 only
    int max_knots;          // H + 1 at most: 64 = one problem per wave segment
    bool certifies;         // the step certificate may run (BatchArgs::certified_steps)
    const char *what;       // how the C-ABI's messages call the shape, with their verb
};
constexpr ShapeInfo kShapes[] = {
    {"biconvex_admm_kernel", false, false, kMaxKnots, true, "diagonal costs are"},
    {"biconvex_admm_bq_kernel", true, true, 64, false, "block costs (Qx_blk / Qf_blk) are"},
    {"biconvex_admm_kq_kernel", true, true, 64, false, "costs between neighbouring knots (Qx_off / Qf_off) are"},
    {"biconvex_admm_cone_kernel", false, true, 64, false, "the Euclidean cone projection (bmpc_cone_t, projection = 1) is"},
    {"biconvex_admm_conef_kernel", false, true, 64, false, "the Euclidean cone projection about contact normals (bmpc_contact_frame_t) is"},
};
constexpr int kNumShapes = sizeof(kShapes) / sizeof(kShapes[0]);
// ... and the struct a shape's arrays reach its kernels in (kDiag: none)
struct NoArgs {};
template <CostShape SHAPE>
using ShapeExtra = std::tuple_element_t<SHAPE, std::tuple<NoArgs, BlockArgs, BandArgs, ConeArgs, ConeFrameArgs>>;

// LDS bytes of a workgroup that holds per_wg problems of H + 1 knots in elements of elem bytes: the zeros, then per problem the
// x_init rows' multipliers and the header and one record per knot (X, P, F, R), then `extra` elements -- and the workgroups of a batch
constexpr size_t launch_lds_bytes(size_t elem, int per_wg, int E, int H, size_t extra = 0) {
    return elem * (kLdsZeros + (size_t)per_wg * ((size_t)kSegLds + (size_t)knot_lds(E) * (size_t)(H + 1)) + extra);
}
// The loop-constants build of the headline kernel (biconvex_admm_body.h: CLDS) parks kLoopConstLds doubles per knot behind the records of
// a wave's two problems: 18 phase constants of the knot's lane in an odd stride (no two lanes of a segment share a bank)
constexpr int kLoopConstLds = 19;
constexpr size_t loop_constants_extra(int H) { return 2 * (size_t)(H + 1) * kLoopConstLds; }
// ... and its wave's LDS bytes: 8 (84 + (78 + 2 x 19) k) for k = H + 1 knots at four feet
constexpr size_t loop_constants_lds_bytes(int E, int H) { return launch_lds_bytes(sizeof(double), 2, E, H, loop_constants_extra(H)); }
// eight such waves share a CU's 160 KB (two per SIMD): 20480 bytes each -- at four feet, k <= 21
constexpr bool loop_constants_fit(int E, int H) { return H >= 1 && 8 * loop_constants_lds_bytes(E, H) <= 160 * 1024; }
// ... and of a workgroup of eight such waves with the mailbox of 16 words behind them (biconvex_admm_body.h: MATES): at most 160 KB - 2432
// bytes + 64 wherever loop_constants_fit holds
constexpr size_t simd_mates_lds_bytes(int E, int H) { return 8 * loop_constants_lds_bytes(E, H) + 64; }
// what mode 2 of set_loop_constants_in_lds ("when it pays") resolves to wherever the build fits: "always", by the measurement in
// EXPERIMENTS.md ("Headline kernel: iterates in registers, loop constants in LDS": 2.82 -> 2.55 ms at B = 4096, H = 20)
#ifndef BMPC_LOOP_CONSTANTS_PAY      // (side-by-side experiment builds: BUNMPC_EXTRA_FLAGS=-DBMPC_LOOP_CONSTANTS_PAY=0)
#define BMPC_LOOP_CONSTANTS_PAY 1
#endif
constexpr bool kLoopConstantsPay = BMPC_LOOP_CONSTANTS_PAY != 0;
// what mode 2 of set_force_foot_pairs ("when it pays") resolves to: "on", by the measurement in EXPERIMENTS.md ("Headline force loop: two
// feet per lane": 2.40 -> 2.21 ms at B = 4096, H = 20, seven alternating pairs, every run below every run of the parent)
#ifndef BMPC_FORCE_FOOT_PAIRS_PAY      // (side-by-side experiment builds: BUNMPC_EXTRA_FLAGS=-DBMPC_FORCE_FOOT_PAIRS_PAY=0)
#define BMPC_FORCE_FOOT_PAIRS_PAY 1
#endif
constexpr bool kForceFootPairsPay = BMPC_FORCE_FOOT_PAIRS_PAY != 0;
// what mode 2 of set_simd_mate_balance ("when it pays") resolves to where the batch fills the chip exactly once (biconvex_launch.hip:
// simd_mates_pay): see EXPERIMENTS.md, "Headline kernel: SIMD-mate waves kept level"
#ifndef BMPC_SIMD_MATES_PAY      // (side-by-side experiment builds: BUNMPC_EXTRA_FLAGS=-DBMPC_SIMD_MATES_PAY=0)
#define BMPC_SIMD_MATES_PAY 1
#endif
constexpr bool kSimdMatesPay = BMPC_SIMD_MATES_PAY != 0;
#ifndef BMPC_SIMD_MATES_RULE     // (measurements: -DBMPC_SIMD_MATES_RULE=0 is the eight-wave geometry without the rule in every mode, as mode 3 is)
#define BMPC_SIMD_MATES_RULE 1
#endif
constexpr bool kSimdMatesRule = BMPC_SIMD_MATES_RULE != 0;
constexpr unsigned launch_grid(int B, int per_wg) { return (unsigned)((B + per_wg - 1) / per_wg); }

// The kernel a batch gets.  Set by plan_launch, except the cost arrays: launch_biconvex_admm adds those.
struct AdmmLaunch {
    int lpp;             // lanes per problem 16 / 21 / 32 / 64, or 128 / 192 / 256: one problem per workgroup of 2 / 3 / 4 waves; 0: the one-problem-per-wave kernel
    bool w2;             // the two-waves-per-SIMD build
    bool steal;          // the work-stealing kernel (lpp 21, harness form, fp64)
    long steal_waves;    // ... its persistent grid
    CostArgs cost;
    bool clds;           // the two-waves build with the certified loops' constants in LDS (32 lanes, four feet, harness form, fp64)
    bool mates = false;        // ... in workgroups of eight waves (biconvex_admm_body.h: MATES)
    bool mate_rule = false;    // ... whose SIMD-mates keep level by priority (false: the geometry alone)
};
// The instantiations of one cost shape, precision and foot count: one translation unit each (bunmpc_amd/build.py lists them).
// launch: the launch plan_launch decided on (a.cmtab and, for the work-stealing kernel, a.queue set); scratch_bytes: the largest
// private-segment bytes per lane over the unit's kernels, -1 on error; loop_constants_resident_waves: see the member
struct AdmmUnit {
    hipError_t (*launch)(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream);
    int (*scratch_bytes)();
    int (*loop_constants_resident_waves)(int H);      // of the unit's loop-constants build, by the occupancy query: waves one CU holds at once; 0: the unit has no such build, -1 on error
    long (*foot_pair_phases)(int reset);              // (wave, force phase) pairs the unit's loop-constants build ran two feet per lane on the current device since the last reset; 0: no such build, -1 on error
};
// The combinations a unit is built for, by kShapes, and each one's accessor: every compilation of biconvex_admm.hip defines the
// explicit specialisation it was built for, and biconvex_launch.hip's table refers to all of them.
constexpr bool unit_is_built(int shape, int precision, int E) {
    return shape >= 0 && shape < kNumShapes && (precision == 0 || (precision == 1 && !kShapes[shape].fp64_only)) && (E == 2 || E == 4);
}
template <CostShape SHAPE, int PRECISION, int E>
const AdmmUnit &admm_unit_of();
// ... of a combination the caller has validated: unit_is_built(shape, precision, n_eff)
const AdmmUnit &admm_unit(CostShape shape, int precision, int n_eff);

// The dispatch switches of the process (the set_* calls below) and what they decide: a pure function of the batch's sizes, the
// chip's SIMD count and the switches -- no HIP call, no pointer of `a` dereferenced.
struct DispatchKnobs {
    int three_per_wave = 2;            // 21-lane segments for 17..21 knots: 0 never, 1 always, 2 when it pays
    int two_per_simd = 2;              // the two-waves-per-SIMD build of the fp64 kernels: 0 never, 1 always, 2 when it pays
    int work_stealing = 1;             // the segment-level work-stealing kernel for num_iters >= 25
    int steal_grid = 0;                // waves of its persistent grid (experiments): 0 = one or two per SIMD
    int latency_max_batch = 1024;      // the one-problem-per-wave kernel up to this many problems
    int exact_step_decisions = 0;      // 1: every step decision from the fp64 sums, in every centroidal kernel; 2: the headline kernel without its lane-local screen (tests)
    int certified_steps = 1;           // the fp64 batch kernels' per-phase step certificate: 0 off, 1 on, 2 force phases only
    int loop_constants_in_lds = 2;     // the headline kernel's build with loop constants in LDS and x_k in registers: 0 never, 1 whenever it fits, 2 when it pays
    int force_foot_pairs = 2;          // ... its certified force loop two feet per lane in eligible phases: 0 never, 1 always, 2 when it pays
    int simd_mate_balance = 2;         // ... in eight-wave workgroups whose SIMD-mates keep level: 0 never, 1 wherever that build is taken, 2 when it pays, 3 as 1 without the rule (measurements)
};
struct LaunchPlan {
    hipError_t status;       // hipErrorInvalidValue: a shape no kernel is built for
    const char *kernel;      // the kernel template's name; null (with hipSuccess): B == 0, nothing to launch
    AdmmLaunch l;
    bool latency;            // the one-problem-per-wave kernel (biconvex_latency.hip)
    int certified_steps;     // BatchArgs::certified_steps of the launch
};
LaunchPlan plan_launch(const BatchArgs &a, CostShape shape, int n_eff, long simds, const DispatchKnobs &knobs);
LaunchPlan plan_launch(const BatchArgs &a, CostShape shape, int n_eff, long simds);      // ... with the process's switches

// Launch the batched ADMM kernel on `stream`: plan_launch with the current device's SIMD count, the device's momentum table (and a
// counter of its work-stealing ring if the plan steals), the "last launch" record, then the unit of (shape, precision, n_eff).
// Returns hipSuccess or the launch error; hipErrorInvalidValue for unsupported shapes (n_eff not 2 or 4, or what the shape's row of
// kShapes excludes -- the C-ABI refuses those with a message first).
hipError_t launch_biconvex_admm(const BatchArgs &a, const CostArgs &cost, int n_eff, hipStream_t stream);

// The one-problem-per-wave mapping (biconvex_latency.hip): fp64, n_eff = 2 or 4, H + 1 <= 21.  plan_launch takes it for
// batches of at most latency_mapping_max_batch() problems that fit.
bool latency_mapping_fits(const BatchArgs &a, int n_eff);
hipError_t launch_biconvex_latency(const BatchArgs &a, int n_eff, hipStream_t stream);
int set_latency_mapping_max_batch(int max_batch);   // returns the old value
int set_three_per_wave(int mode);                    // 21-lane segments for 17..21 knots: 0 never, 1 always, 2 when it pays (default); returns the old value
int set_two_waves_per_simd(int mode);               // the two-waves-per-SIMD build of the fp64 batch kernel: 0 never, 1 always, 2 when it pays (default); returns the old value
int biconvex_last_waves_per_simd();                  // of the calling host thread's latest launch (1 or 2)
int set_steal_grid(int waves);                       // waves of the work-stealing kernel's persistent grid (experiments; 0 = what the chip holds); returns the old value
int set_work_stealing(int on);                       // the segment-level work-stealing kernel for num_iters >= 25 (default on); returns the old value
int biconvex_last_lanes_per_problem();               // of the calling host thread's latest launch: 16 / 21 / 32 / 64, 0 = one problem per wave
int set_exact_step_decisions(int on);                // 1: every step decision from the fp64 sums, in every centroidal kernel; 2: fp32 decisions without the headline kernel's lane-local screen; returns the old value
int set_loop_constants_in_lds(int mode);             // the headline kernel's certified loops with their constants in LDS and x_k in registers: 0 never, 1 whenever it fits, 2 when it pays (default); returns the old value
int set_force_foot_pairs(int mode);                  // the loop-constants build's certified force loop with two feet per lane where a phase is eligible: 0 never, 1 always, 2 when it pays (default); returns the old value
int set_simd_mate_balance(int mode);                 // the loop-constants build in eight-wave workgroups whose SIMD-mates keep level by priority: 0 never, 1 wherever that build is taken, 2 when it pays (default), 3 the geometry without the rule; returns the old value
int biconvex_last_block_size();                      // threads per workgroup of the calling host thread's latest launch_biconvex_admm (0: the one-problem-per-wave kernel)
int set_certified_steps(int on);                     // the fp64 batch kernels' per-phase step certificate: 0 off, 1 on (default), 2 force phases only; returns the old value

// Lane-exchange self test (DPP shifts and segment sums used by the kernel).
// out must hold 12*64 doubles.
hipError_t launch_lane_selftest(const double *in, double *out, hipStream_t stream);
// The lane-helper probe (lane_probe.hip; bmpc_probe_lanes): rows of 64 words a wave of `group` reads and writes (false: no such group), and
// the launch of `waves` waves on device arrays of waves * nin * 64 and waves * nout * 64 words.
bool lane_probe_words(int group, int *nin, int *nout);
hipError_t launch_lane_probe(int group, const unsigned long long *in, unsigned long long *out, long waves, hipStream_t stream);

// Name of the kernel symbol for a given H (for profiling / bench reports).
const char *biconvex_kernel_name(int H, int raw);
// ... and of the kernel the calling host thread's latest launch_biconvex_admm actually took
const char *biconvex_last_kernel_name();

}  // namespace bunmpc
