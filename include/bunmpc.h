/*
 * include/bunmpc.h -- C-ABI of libbunmpc_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the BiConvex MPC solve path of Atarilab/BUNMPC.  The
 * reference crosses Python -> C++ through three pybind11 modules
 * (iterative_supervised_learning/srcpy/...); each entry point below names the
 * binding line it replaces.  Plain pointers and sizes only; every function that
 * can fail returns an int status and never throws:
 *      BMPC_OK 0, BMPC_BAD_ARG 1, BMPC_DIVERGED 2 (NaN in the dynamics violation),
 *      BMPC_DEVICE_ERROR 3 (HIP error; text via bmpc_last_error()).
 * Matrices are row-major doubles unless stated.  The single-problem handles keep
 * the reference's call semantics (append-style set_contact_plan, persistent FISTA
 * step constants, state surviving between optimize calls); the *_batch entry
 * points are additive and solve many independent problems in one kernel launch.
 * All compute runs on the GPU: there is no CPU fallback in this library.
 */
#ifndef BUNMPC_H
#define BUNMPC_H

#ifdef __cplusplus
extern "C" {
#endif

#define BMPC_OK 0
#define BMPC_BAD_ARG 1
#define BMPC_DIVERGED 2
#define BMPC_DEVICE_ERROR 3

/* library / device ----------------------------------------------------------- */
int bmpc_abi_version(void);
int bmpc_abi_minor_version(void);            /* additions within an ABI version: 1 = bmpc_batch_t ends in cert_phases; 2 = the
                                              * Euclidean cone projection (bmpc_cone_t and the calls beside it) */
int bmpc_batch_struct_size(void);            /* sizeof(bmpc_batch_t), to catch binding drift  */
const char *bmpc_last_error(void);           /* thread-local text of the last failure   */
int bmpc_device_count(int *count);           /* hipGetDeviceCount                        */
int bmpc_set_device(int device);             /* hipSetDevice for the calling thread      */
/* DPP / permlane self test of the lane exchanges the kernels rely on; 0 = pass.     */
int bmpc_selftest_lanes(void);
/* TEST ONLY.  The lane helpers of the centroidal kernels (bunmpc_amd/csrc/biconvex_lanes.h) called on the caller's inputs, one group of
 * helpers per call, so that a test can hold each to a model bit for bit (tests/lanes_np.py).  in / out are HOST arrays of 64-bit
 * words.  A wave of 64 lanes is one test case: in is [waves][NIN][64], out is [waves][NOUT][64], word [w][k][lane]; a double is its bit
 * pattern, a float or a 32-bit integer sits in the low half of its word (high half: ignored in, zero out), a flag is 0 / 1.
 * in_bytes = waves * NIN * 512 with waves in 1 .. 2^20, out_bytes = waves * NOUT * 512.  An unknown group, a null pointer or sizes that
 * do not fit the group's layout: BMPC_BAD_ARG, before any device call.  "lane 0's" below: the scalar is read from word [w][k][0].
 *   SUM64 (NIN 2: a, b doubles; NOUT 16): for L = 16, 21, 32, 64, at out 4 i .. 4 i + 3: seg_sum<L>(a); seg_sum2<L>(a, b)'s two results;
 *       seg_sum1<L>(a).  (L = 21: the last three are meaningful at lanes 16, 32, 48 only.)
 *   SUM32 (NIN 2: a, b floats; NOUT 9): for L = 16, 32, 64, at out 3 i .. 3 i + 2: seg_sum2_f32<L>(a, b)'s two results; seg_sum1_f32<L>(a).
 *   SHIFT (NIN 2: a double, a float; NOUT 4): from_prev, from_next of the double; from_prev, from_next of the float.
 *   MASK  (NIN 2: lane 0's masks m, need; NOUT 9, wave-uniform but for out 7): seg_uniform<21>(m & seg_desig<21>()); seg_covered<16>,
 *       <32>, <64>(m, need) as flags; d0, d1 of seg_dead32(need); seg_covered32(m, d0, d1); out 7: lanes(m) as the lane's flag; the
 *       ballot of lanes(m).
 *   THETA (NIN 2: tol2, floor2 doubles; NOUT 1): lane j's word is screen_theta(tol2[j], floor2[j]) -- 64 wave-uniform evaluations.
 *   ARITH (NIN 7: doubles a, b, c; flags word: low half the mask m of keep_if, bit 32 the flag ok; floats fa, fb, fc; NOUT 17):
 *       0 keep_if(a, m); 1 keep_if(fa, m); 2 fma3(a, b, c); 3 fma3_s(lane 0's a through uniform_load, b, c); 4 clamp_box(v = a, lo = b,
 *       hi = c); 5 clamp_box(fa, fb, fc); 6 .. 11 lds_block<6> of the record (a, b, c, a, b, c) the lane wrote to LDS, under ok;
 *       12 ldz<double>(a, ok); 13 ldz<float>(a, ok); 14 uniform_load(b's 64 words, lane); 15 fast_div(a, b); 16 fast_div(fa, fb).
 *   BANDED (NIN 4: g2, cv doubles; lane 0's Lh, tol2; NOUT 3, wave-uniform flags): banded_decisions' return value, retry, finished. */
#define BMPC_PROBE_SUM64 0
#define BMPC_PROBE_SUM32 1
#define BMPC_PROBE_SHIFT 2
#define BMPC_PROBE_MASK 3
#define BMPC_PROBE_THETA 4
#define BMPC_PROBE_ARITH 5
#define BMPC_PROBE_BANDED 6
int bmpc_probe_lanes(int group, const void *in, long in_bytes, void *out, long out_bytes);

/* gait_planner_cpp.GaitPlanner --------------------------------------------------
 * srcpy/gait_planner/py_gait_planner.cpp:19-35 over src/gait_planner/gait_planner.cpp */
typedef struct bmpc_gait bmpc_gait_t;
bmpc_gait_t *bmpc_gait_create(double gait_period, const double *stance_percent,
                              const double *phase_offset, int n_eff, double step_height); /* :22 */
void bmpc_gait_destroy(bmpc_gait_t *g);
int bmpc_gait_n_eff(const bmpc_gait_t *g);
int bmpc_gait_get_phase(bmpc_gait_t *g, double t, int foot_id, int *phase);             /* :25 */
int bmpc_gait_get_phase_all(bmpc_gait_t *g, double t, int *phase);                      /* :26 */
int bmpc_gait_get_phi(bmpc_gait_t *g, double t, int foot_id, double *phi);              /* :27 */
int bmpc_gait_get_phi_all(bmpc_gait_t *g, double t, double *phi);                       /* :28 */
int bmpc_gait_get_percent_in_phase(bmpc_gait_t *g, double t, int foot_id, double *pct); /* :29-30 */
int bmpc_gait_get_percent_in_phase_all(bmpc_gait_t *g, double t, double *pct);          /* :31-32 */
/* plan: rows x n_eff ints, row i = get_phase_all(t + i*dt)                             :33 */
int bmpc_gait_get_contact_phase_plan(bmpc_gait_t *g, int rows, double t, double dt, int *plan);
int bmpc_gait_set_step_height(bmpc_gait_t *g, double step_height);                      /* :34 */
int bmpc_gait_set_stance_percent(bmpc_gait_t *g, double lf, double lh, double rf, double rh); /* :35 */

/* biconvex_mpc_cpp.BiconvexMP ----------------------------------------------------
 * srcpy/motion_planner/biconvex.cpp:19-44 over src/motion_planner/biconvex.cpp */
typedef struct bmpc_biconvex bmpc_biconvex_t;
bmpc_biconvex_t *bmpc_biconvex_create(double m, int n_col, int n_eff);                  /* :20 */
void bmpc_biconvex_destroy(bmpc_biconvex_t *h);
int bmpc_biconvex_n_col(const bmpc_biconvex_t *h);
int bmpc_biconvex_n_eff(const bmpc_biconvex_t *h);
/* cnt_plan: n_eff x 4 rows [flag,x,y,z]; appended (H calls per solve)                  :21 */
int bmpc_biconvex_set_contact_plan(bmpc_biconvex_t *h, const double *cnt_plan, double dt);
int bmpc_biconvex_set_rotation_matrix_f(bmpc_biconvex_t *h, const double *R3x3);        /* :22 */
/* dense debugging copies; A_x: 9(H+1) x 3EH, A_f: 9(H+1) x 9(H+1)                      :23-26 */
int bmpc_biconvex_return_A_x(bmpc_biconvex_t *h, const double *X, double *A_x);
int bmpc_biconvex_return_b_x(bmpc_biconvex_t *h, const double *X, double *b_x);
int bmpc_biconvex_return_A_f(bmpc_biconvex_t *h, const double *F, const double *x_init, double *A_f);
int bmpc_biconvex_return_b_f(bmpc_biconvex_t *h, const double *F, const double *x_init, double *b_f);
/* Q is passed as its diagonal (the shim rejects off-diagonal entries)                  :27,29 */
int bmpc_biconvex_set_cost_x(bmpc_biconvex_t *h, const double *Q_diag, const double *q);
int bmpc_biconvex_set_cost_f(bmpc_biconvex_t *h, const double *Q_diag, const double *q);
int bmpc_biconvex_create_cost_X(bmpc_biconvex_t *h, const double *W_X, const double *W_X_ter,
                                const double *X_ter, const double *X_nom);              /* :28 */
int bmpc_biconvex_create_cost_F(bmpc_biconvex_t *h, const double *W_F);                 /* :30 */
int bmpc_biconvex_set_bounds_x(bmpc_biconvex_t *h, const double *lb, const double *ub); /* :31 */
int bmpc_biconvex_set_bounds_f(bmpc_biconvex_t *h, const double *lb, const double *ub); /* :32 */
/* b: rows x cols (cols must be 6, rows >= n_col)                                       :33 */
int bmpc_biconvex_create_bound_constraints(bmpc_biconvex_t *h, const double *b, int rows, int cols,
                                           double fx_max, double fy_max, double fz_max);
int bmpc_biconvex_set_rho(bmpc_biconvex_t *h, double rho);                              /* :34 */
int bmpc_biconvex_return_opt_x(bmpc_biconvex_t *h, double *X);      /* 9(H+1)           :35 */
int bmpc_biconvex_return_opt_f(bmpc_biconvex_t *h, double *F);      /* 3EH              :36 */
int bmpc_biconvex_return_opt_p(bmpc_biconvex_t *h, double *P);      /* 9(H+1)           :37 */
int bmpc_biconvex_return_opt_com(bmpc_biconvex_t *h, double *com);  /* (H+1) x 3        :38 */
int bmpc_biconvex_return_opt_mom(bmpc_biconvex_t *h, double *mom);  /* (H+1) x 6        :39 */
int bmpc_biconvex_set_warm_start_vars(bmpc_biconvex_t *h, const double *X, const double *F,
                                      const double *P);                                 /* :41 */
/* returns BMPC_DIVERGED after writing NaNs, like the reference prints and returns      :42 */
int bmpc_biconvex_optimize(bmpc_biconvex_t *h, const double *x_init, int num_iters);
int bmpc_biconvex_dyn_viol_hist_size(const bmpc_biconvex_t *h);                         /* :43 */
int bmpc_biconvex_return_dyn_viol_hist(const bmpc_biconvex_t *h, double *hist);
int bmpc_biconvex_collect_statistics(bmpc_biconvex_t *h);                               /* :44 */
/* additive: FISTA step constants carried by the handle (fista.hpp:52), solver counters
 * of the last optimize: {admm iters, F-FISTA iters, X-FISTA iters, F retries, X retries, status} */
int bmpc_biconvex_get_step_constants(const bmpc_biconvex_t *h, double *L_x, double *L_f);
int bmpc_biconvex_set_step_constants(bmpc_biconvex_t *h, double L_x, double L_f);
int bmpc_biconvex_last_stats(const bmpc_biconvex_t *h, int *stats6);
/* not bound by the reference but public on the C++ class (biconvex.hpp:131-137) */
int bmpc_biconvex_set_friction_coefficient(bmpc_biconvex_t *h, double mu);
int bmpc_biconvex_set_robot_mass(bmpc_biconvex_t *h, double m);

/* batch of independent solves (additive) ------------------------------------------
 * One kernel launch = B x BiConvexMP::optimize.  Array shapes, batch outermost:
 *   cnt_plan [B][H][E][4], dt [B][H], x_init [B][9]
 *   harness form (raw = 0): W_X [.][9H], W_X_ter [.][9], W_F [.][3EH], bounds [.][H][6]
 *       with batch strides s* in doubles (0 = one copy shared by the batch; at most 2^26),
 *       X_nom [B][9H], X_ter [B][9]      -- the kernel applies create_cost_X /
 *       create_cost_F / create_bound_constraints (biconvex.cpp:27-78) itself
 *   raw form (raw = 1): Qx, qx, lbx, ubx [B][9(H+1)], Qf [B][3EH], qf [B][3EH] or NULL
 *   X [B][9(H+1)], F [B][3EH], P [B][9(H+1)], L_x [B], L_f [B]   in: warm start, out: result
 *   dyn_viol [B] or NULL, hist [B][num_iters] or NULL, stats [B][6] or NULL
 *   trace [B][num_iters][4] ints or NULL: running totals {F-step FISTA iterations, X-step FISTA iterations, F-step retries,
 *       X-step retries} after every ADMM iteration that ran (rows of iterations that did not run are not written) -- with hist
 *       the solve's discrete path per ADMM iteration, what the prefix-parity tests compare with the CPU oracle's
 *   cert_phases [B][2] ints or NULL: per problem, how many force phases and how many motion phases ran the certified FISTA loop
 *       from their first iteration (bmpc_set_certified_steps).  Written by the two-waves-per-SIMD build of the batch kernel at 32
 *       lanes per problem, four feet, harness form (the benchmark's kernel); every other kernel leaves the array as it is.
 *   A caller built against an older header must zero-initialise the whole struct (bmpc_batch_defaults does) and check
 *   bmpc_batch_struct_size() == sizeof(bmpc_batch_t).
 *   Shapes: n_eff in {2, 4}; n_col + 1 <= 256 knots (up to 64: 4 / 3 / 2 / 1 problems per wave, fp64 or fp32 iterates; 65 .. 256: one
 *   problem per workgroup of two .. four waves, fp64 -- the horizons of the reference's examples/analysis/solve_times_test.py).
 */
typedef struct {
    int B, n_col, n_eff, raw;
    int num_iters, maxit;
    int cold_start;   /* 0: X/F/P/L_x/L_f on entry are the warm start (set_warm_start_vars; L_ persists, fista.hpp:52).
                         1: a FRESH KinoDynMP per problem: ignore X/F/P/L_x/L_f on entry -- X = tile(x_init), F = 0, P = 0
                            (KinoDynMP::set_warm_starts, kino_dyn.cpp:83-99) AND L = BMPC_L0_X / BMPC_L0_F (the constructor's
                            values, biconvex.cpp:20-21): independent batch elements.
                         2: the NEXT optimize call of the same KinoDynMP objects: iterates reset as in 1, L_x / L_f taken from
                            the arrays (the reference never resets FISTA's L_ between calls): replans of the same rollouts. */
    int precision;    /* 0: fp64 arithmetic (reference behaviour).  1: fp32 iterates / operators / projections with
                         every accept / exit decision and the dynamics violation reduced in fp64; harness form
                         only; arrays stay fp64 in memory (BASELINE config 3) */
    double m, rho, mu, beta, tol, exit_tol;
    const double *cnt_plan, *dt, *x_init;
    const double *W_X, *W_X_ter, *W_F, *bounds, *X_nom, *X_ter;
    long sW_X, sW_X_ter, sW_F, sbounds;
    const double *Qx, *qx, *lbx, *ubx, *Qf, *qf;
    double *X, *F, *P, *L_x, *L_f;
    double *dyn_viol, *hist;
    int *stats;
    int *trace;       /* ABI version 2 */
    int *cert_phases; /* ABI version 2, minor version 1 */
} bmpc_batch_t;

/* reference defaults: rho 1e5 (biconvex.hpp:148), mu 1, beta 1.5, tol 1e-5, exit_tol 1e-3,
 * maxit 150 (biconvex.hpp:152-160); L0 constants 2.25e6 / 506.25 (biconvex.cpp:20-21) */
void bmpc_batch_defaults(bmpc_batch_t *d);
#define BMPC_L0_X 2.25e6
#define BMPC_L0_F 506.25

/* all pointers are DEVICE pointers; asynchronous on hip_stream (a hipStream_t, NULL = default) */
int bmpc_biconvex_solve_batch_device(const bmpc_batch_t *d, void *hip_stream);
/* all pointers are HOST pointers; copies in, solves, copies out, synchronises */
int bmpc_biconvex_solve_batch_host(const bmpc_batch_t *d);
/* Kernel selection (no effect on the discrete path; values equal to rounding): batches of at most max_batch problems with
 * n_col + 1 <= 21 knots in fp64 are solved ONE PROBLEM PER WAVE (knots x component groups across the lanes: the dependent
 * chain of a solve is ~2.3x shorter), larger ones one knot per lane with 4 / 2 / 1 problems per wave.  Default 1024 (one
 * wave per SIMD of an MI355X); 0 = never.  Returns the old value. */
int bmpc_set_latency_mapping_max_batch(int max_batch);
/* Horizons of 17..21 knots (n_col = 16..20: the headline shape) in fp64 can run THREE problems per wave, in 21-lane segments,
 * instead of two in 32-lane segments (same iterates; the segment sums behind the step decisions are added in another order, as
 * between any two of the mappings).  mode 0: never, 1: always, 2 (default): when it finishes the batch sooner -- fewer rounds of
 * waves over the chip's SIMDs (not at B = 4096 on an MI355X: 1366 waves or 2048, two rounds either way; at B = 3072 or 6144 it
 * saves a round), or num_iters >= 25 (iteration counts differ per problem).  Returns the old value. */
int bmpc_set_three_per_wave(int mode);
/* With many ADMM iterations (num_iters >= 25) the early exit (biconvex.cpp:111-114) makes the iteration counts differ per problem
 * (34 .. 100 at the reference's num_iters = 100).  The three-per-wave kernel then runs as a PERSISTENT grid of one wave per SIMD in
 * which a segment whose problem has finished stores its results and takes the next unsolved problem from a device counter
 * ("biconvex_admm_steal_kernel"): the batch takes the sum of the problems' iterations over the segments, not the per-wave maxima.
 * A problem's result does not depend on it.  on = 0: never (a test switch).  Default 1.  Returns the old value. */
int bmpc_set_work_stealing(int on);
/* waves of that persistent grid (an experiment switch; 0, the default: as many as the chip holds at once).  Returns the old value. */
int bmpc_set_steal_grid(int waves);
/* The fp64 batch kernel (16 / 32 / 64 lanes per problem) exists in two builds: for ONE wave per SIMD (FISTA iterates in registers,
 * ~290 of them) and for TWO (256 registers: x_k and its affine image rest in LDS between the iterations; same operations in the
 * same order, bit-identical results).  A lone wave of the second build is the slower one, two of them on a SIMD cover each
 * other's latencies.  mode 0: never the second, 1: always, 2 (default): when the batch needs more waves than the chip has SIMDs
 * (B = 4096 at n_col = 20 on an MI355X: 2048 waves over 1024 SIMDs).  Returns the old value. */
int bmpc_set_two_waves_per_simd(int mode);
/* lanes per problem of the calling host thread's latest batch solve: 16 / 21 / 32 / 64 (128 / 192 / 256: a workgroup of 2 / 3 / 4 waves), 0 = the one-problem-per-wave kernel */
int bmpc_biconvex_last_lanes_per_problem(void);
/* ... and the waves per SIMD its kernel was built for (1 or 2) */
int bmpc_biconvex_last_waves_per_simd(void);
/* Two centroidal kernels take the decisions of a FISTA step (retry, fista.cpp:16; exit, fista.cpp:29) from fp32 sums whenever every
 * comparison of the wave's live problems is clear of its threshold by 1e-5 relative, from the fp64 sums and the reference expression
 * otherwise: the one-problem-per-wave kernel, and the two-waves-per-SIMD build of the batch kernel at 32 lanes per problem, four feet,
 * harness form (the benchmark's kernel).  Every other kernel always uses the fp64 sums.  The benchmark's kernel
 * also screens the iterations of its certified loops lane by lane: a lane whose own share of the squared step is above
 * max(tol^2, floor) (1 + 2^-40) settles its problem's exit and floor decisions without any sum.
 *   on = 0 (default): the screen, then the fp32 decisions, then the fp64 sums;
 *   on = 1: every decision from the fp64 sums, no screen, in both kernels (what the A/B tests compare against);
 *   on = 2: the benchmark's kernel takes the fp32 decisions without the screen; the one-problem-per-wave kernel has no screen and
 *           reads any non-zero value as 1.
 * A test switch: results must be bit-identical under every value.  Returns the old value. */
int bmpc_set_exact_step_decisions(int on);
/* The fp64 batch kernels skip FISTA's backtracking test for a whole force step (one ADMM iteration's force-QP loop) of a wave whose
 * live problems all carry a certificate that the test cannot fire: a diagonally scaled Gershgorin bound of the step's Hessian
 * below (L/2)(1 - 2^-6).  The benchmark's kernel (two waves per SIMD, 32 lanes per problem, four feet, harness
 * form) does the same for the motion step, whose bound couples neighbouring knots.  on = 0: every step is tested; 1 (default): both
 * steps where a kernel has them; 2: the force step only (test switches: results must be bit-identical whatever the value).
 * Returns the old value. */
int bmpc_set_certified_steps(int on);
/* The benchmark's kernel (two waves per SIMD, 32 lanes per problem, four feet, harness form, fp64, diagonal costs) exists in a second
 * two-waves build whose certified FISTA loops keep x_k and its image in registers and read 18 constants of the phase from LDS instead
 * (DESIGN.md section 4): same operations in the same order, bit-identical results.  Its wave needs bmpc_loop_constants_lds_bytes of LDS,
 * and eight waves share a CU's 160 KB: bmpc_loop_constants_fit, n_col = 16 .. 20 at four feet.  mode 0: never that build; 1: wherever
 * the two-waves build is taken and it fits; 2 (default): when it pays -- which the measurement recorded in EXPERIMENTS.md resolves to
 * "wherever it fits" (B = 4096, n_col = 20: 2.82 -> 2.55 ms).  Only the kernel behind the record changes: bmpc_biconvex_last_kernel_name / _lanes_per_problem / _waves_per_simd and the
 * same fields of bmpc_biconvex_plan_launch report what they report for the two-waves build; the plan's loop_constants_in_lds tells
 * them apart.  Returns the old value. */
int bmpc_set_loop_constants_in_lds(int mode);
/* LDS bytes of a wave of that build for n_col + 1 knots (two problems per wave; -1 for another n_eff or n_col < 1) and whether eight of
 * them fit a CU: 8 (84 + (78 + 2 x 19) (n_col + 1)) <= 20480 at four feet.  Pure functions. */
long bmpc_loop_constants_lds_bytes(int n_eff, int n_col);
int bmpc_loop_constants_fit(int n_eff, int n_col);
/* Waves of that build one CU holds at once at this n_col, as the runtime's occupancy query answers for the loaded code object and the
 * current device: 8 is what two waves per SIMD need (at n_col = 20 the LDS of eight waves fills the CU to the allocation granule).
 * -1 (BMPC_BAD_ARG) where the build does not fit, or on error.  Needs a GPU. */
int bmpc_loop_constants_resident_waves(int n_col);
/* Scratch (private-segment) bytes per lane of the fp32 kernels as the loaded code object reports them, -1 on error.  0 is what
 * the build is set up for (bunmpc_amd/build.py: their translation unit is compiled without the SLP vectoriser); a compiler that
 * spills again shows up here, and in 4x the HBM traffic. */
int bmpc_biconvex_fp32_scratch_bytes(void);
/* The largest scratch (private-segment) bytes per lane over the batch-kernel instantiations of one foot count (n_eff 2 or 4) and
 * precision (0: fp64 -- one knot per lane at every lanes-per-problem and build, one problem per workgroup, work stealing; 1: fp32),
 * as the loaded code object reports them; -1 (BMPC_BAD_ARG) for another n_eff or precision, or on error. */
int bmpc_biconvex_kernel_scratch_bytes(int n_eff, int precision);
/* symbol-name prefix of the kernel that serves (n_col, raw), for profiles */
const char *bmpc_biconvex_kernel_name(int n_col, int raw);
/* which kernel the calling host thread's latest batch solve was dispatched to: "biconvex_latency_kernel" (one problem per wave),
 * "biconvex_admm_kernel" or "biconvex_admm_kernel_f32" (one knot per lane), "biconvex_admm_bq_kernel" (block costs),
 * "biconvex_admm_kq_kernel" (costs between neighbouring knots); "" before the first solve */
const char *bmpc_biconvex_last_kernel_name(void);
/* Which kernel a batch solve of descriptor d would be dispatched to on a chip of `simds` SIMDs (an MI355X: 256 CUs x 4 = 1024), with
 * the process's current dispatch switches (the bmpc_set_* calls above).  cost_shape 0: diagonal costs (bmpc_biconvex_solve_batch_*),
 * 1: block costs, 2: costs between neighbouring knots.  A pure function: it reads only the scalar fields of d (B, n_col, n_eff, raw,
 * precision, num_iters, maxit, cold_start, the strides) -- no pointer in d is looked at, let alone dereferenced -- and makes no GPU
 * call, so it runs on a machine without one.  status: BMPC_OK, or BMPC_BAD_ARG (also returned; bmpc_last_error explains) for a shape
 * the solve calls refuse.  lanes_per_problem / waves_per_simd / kernel: what bmpc_biconvex_last_* report after the solve, except
 * waves_per_simd = 0 for the one-problem-per-wave kernel (which leaves that record alone); kernel is "" when B == 0 (no launch).
 * steal / steal_waves: the work-stealing kernel and its persistent grid. */
typedef struct {
    int status;
    int lanes_per_problem;
    int waves_per_simd;
    int steal;
    long steal_waves;
    const char *kernel;
    int loop_constants_in_lds;      /* 1: the build of bmpc_set_loop_constants_in_lds behind this record */
} bmpc_launch_plan_t;
int bmpc_biconvex_plan_launch(const bmpc_batch_t *d, int cost_shape, long simds, bmpc_launch_plan_t *out);

/* Per-knot block-diagonal costs (additive) --------------------------------------------------------------------------------
 * The reference's set_cost_x / set_cost_f take a sparse matrix (biconvex.hpp:54-60) and ProblemData uses all of it
 * (problem.cpp:31-56).  Here Q may be block-diagonal per knot: a symmetric 9 x 9 block per knot for X, a symmetric 3E x 3E block per
 * knot for F -- weights in a rotated frame, terms that couple the feet of a knot, CoM position-velocity coupling.  Blocks are
 * row-major and must be symmetric (the gradient 2 Q y and the test's (y1 + y0)'Q d agree for symmetric Q only; the host entry
 * points check it, the device entry point cannot).  Anything that couples different knots cannot be expressed.
 * Either pointer may be NULL: that side uses the batch descriptor's diagonal (d->Qx / d->Qf, which the other side then does not
 * need).  With both NULL the calls are the plain ones.  Strides in doubles: 0 = one set of blocks shared by the batch, otherwise at
 * least one problem's blocks and at most 2^26.
 * Built for: raw form (raw = 1), fp64 (precision = 0), n_col + 1 <= 64 knots, n_eff in {2, 4}; anything else is BMPC_BAD_ARG with a
 * message that names the limit.  Such a batch runs "biconvex_admm_bq_kernel" (one knot per lane, 16 / 21 / 32 / 64 lanes per
 * problem, one wave per SIMD) at every batch size and num_iters; every FISTA step is tested on fp64 sums (no step certificate, no
 * fp32 step decisions), so bmpc_set_certified_steps, bmpc_set_exact_step_decisions, bmpc_set_work_stealing and
 * bmpc_set_two_waves_per_simd do not touch it. */
typedef struct {
    const double *Qx_blk; long sQx_blk;   /* [.][n_col+1][9][9] */
    const double *Qf_blk; long sQf_blk;   /* [.][n_col][3E][3E] */
} bmpc_block_cost_t;
int bmpc_block_cost_struct_size(void);       /* sizeof(bmpc_block_cost_t), to catch binding drift */
int bmpc_biconvex_solve_batch_blocks_device(const bmpc_batch_t *d, const bmpc_block_cost_t *c, void *hip_stream);
int bmpc_biconvex_solve_batch_blocks_host(const bmpc_batch_t *d, const bmpc_block_cost_t *c);
/* The handle's cost as blocks: Q_blk [n_col+1][9][9] / [n_col][3E][3E], q as in set_cost_x / set_cost_f.  optimize then takes the
 * block kernel while either side has blocks; bmpc_biconvex_set_cost_x / _f (or create_cost_X / _F) return that side to its diagonal. */
int bmpc_biconvex_set_cost_x_blocks(bmpc_biconvex_t *h, const double *Q_blk, const double *q);
int bmpc_biconvex_set_cost_f_blocks(bmpc_biconvex_t *h, const double *Q_blk, const double *q);
/* The largest scratch (private-segment) bytes per lane over the block-cost kernels of one foot count (n_eff 2 or 4), as the loaded
 * code object reports them; -1 for another n_eff, or on error.  (bmpc_biconvex_kernel_scratch_bytes covers the other kernels.) */
int bmpc_biconvex_block_kernel_scratch_bytes(int n_eff);

/* Costs between neighbouring knots ("band" costs, additive) -----------------------------------------------------------------
 * A force-rate term sum_t (F_{t+1} - F_t)' R_t (F_{t+1} - F_t), or the same difference on rows of X (CoM acceleration, momentum
 * rate), is D' R D with D the first difference over the knots: a Q that is block-tridiagonal over the knots with DIAGONAL
 * off-diagonal blocks.  That class is taken here:
 *     Q[(t, i), (t, i)]     = the per-knot diagonal, d->Qx / d->Qf as ever
 *     Q[(t, i), (t + 1, i)] = Q[(t + 1, i), (t, i)] = off[t][i]        (any sign; Q = diag + D' R D: diag[t] += R[t-1] + R[t], off[t] = -R[t])
 * Either pointer may be NULL: that side has no coupling.  With c NULL or both pointers NULL the calls are the plain ones.  Strides
 * in doubles: 0 = one set of weights shared by the batch, otherwise at least one problem's weights and at most 2^26.
 * Not expressible: off-diagonal blocks that are not diagonal, coupling beyond the next knot, and coupling together with per-knot
 * blocks (bmpc_block_cost_t) on either side.
 * Built for: raw form (raw = 1), fp64 (precision = 0), n_col + 1 <= 64 knots, n_eff in {2, 4}; anything else is BMPC_BAD_ARG with a
 * message that names the limit.  Such a batch runs "biconvex_admm_kq_kernel" (one knot per lane, 16 / 21 / 32 / 64 lanes per
 * problem, one wave per SIMD) at every batch size and num_iters; every FISTA step is tested on fp64 sums (no step certificate, no
 * fp32 step decisions), so bmpc_set_certified_steps, bmpc_set_exact_step_decisions, bmpc_set_work_stealing and
 * bmpc_set_two_waves_per_simd do not touch it. */
typedef struct {
    const double *Qx_off; long sQx_off;   /* [.][n_col][9]        weight between knots t and t + 1 of X */
    const double *Qf_off; long sQf_off;   /* [.][n_col - 1][3E]   ... of F                              */
} bmpc_band_cost_t;
int bmpc_band_cost_struct_size(void);        /* sizeof(bmpc_band_cost_t), to catch binding drift */
int bmpc_biconvex_solve_batch_band_device(const bmpc_batch_t *d, const bmpc_band_cost_t *c, void *hip_stream);
int bmpc_biconvex_solve_batch_band_host(const bmpc_batch_t *d, const bmpc_band_cost_t *c);
/* The handle's cost with coupling: Q_diag [n_col+1][9] / [n_col][3E] and q as in set_cost_x / set_cost_f, Q_off [n_col][9] /
 * [n_col-1][3E] (NULL: none).  optimize then takes the band kernel while either side has coupling; bmpc_biconvex_set_cost_x / _f
 * (or create_cost_X / _F) return that side to its diagonal.  A handle that carries coupling on one side and blocks on either is
 * refused by optimize (BMPC_BAD_ARG). */
int bmpc_biconvex_set_cost_x_band(bmpc_biconvex_t *h, const double *Q_diag, const double *Q_off, const double *q);
int bmpc_biconvex_set_cost_f_band(bmpc_biconvex_t *h, const double *Q_diag, const double *Q_off, const double *q);
/* The largest scratch (private-segment) bytes per lane over the band-cost kernels of one foot count (n_eff 2 or 4), as the loaded
 * code object reports them; -1 for another n_eff, or on error. */
int bmpc_biconvex_band_kernel_scratch_bytes(int n_eff);

/* Euclidean projection onto the friction cone, per-foot friction coefficients (additive, opt-in) ------------------------------
 * The force QP's projection is by default the reference's "SoC" step (fista.cpp:52-70), which compares the SQUARED tangential norm
 * with mu fz, zeroes every force with fz < 0 and is expansive on its cone branch.  projection = 1 replaces it by the nearest point of
 * the cone |f_xy| <= mu fz, per foot and knot, with s2 = fx^2 + fy^2 of the gradient step (fx, fy, fz):
 *     fz <= 0 and mu^2 s2 <= fz^2   -> (0, 0, 0)          (the polar cone; wins at the origin)
 *     fz >= 0 and s2 <= mu^2 fz^2   -> unchanged
 *     otherwise                     -> s = sqrt(s2), t = (mu s + fz) / (mu^2 + 1): (fx mu t / s, fy mu t / s, t)
 * Everything else of the solve is unchanged: gradient, backtracking test, momentum, exits, ADMM.  As under the reference's
 * projection, the force bounds of create_bound_constraints / set_bounds_f are not applied.  The cone's axis is world z unless the call
 * carries contact normals (bmpc_contact_frame_t, below); set_rotation_matrix_f on its own stays stored and unused.
 * mu: friction coefficients [.][n_col][n_eff], each finite and > 0 (the host entry point and the handle's setter check that, the
 * device entry point cannot), or NULL: every foot has bmpc_batch_t's scalar mu.  smu: batch stride in doubles, 0 = one set shared by
 * the batch, otherwise at least n_col * n_eff and at most 2^26.
 * c == NULL, or projection == 0 with mu == NULL, is the plain call: same kernel, same bits.  BMPC_BAD_ARG with a message naming the
 * limit: projection == 0 with a mu array (the kernels of the reference's projection take the scalar), projection other than 0 / 1,
 * fp32 (precision = 1), n_col + 1 > 64 knots, n_eff other than 2 or 4, a stride outside the rule above.  Both forms (raw = 0 / 1, with
 * and without qf) are built.  Such a batch runs "biconvex_admm_cone_kernel" (one knot per lane, 16 / 21 / 32 / 64 lanes per problem, one
 * wave per SIMD) at every batch size and num_iters; every FISTA step is tested on fp64 sums (no step certificate, no fp32 step
 * decisions), so bmpc_set_certified_steps, bmpc_set_exact_step_decisions, bmpc_set_work_stealing, bmpc_set_two_waves_per_simd and
 * bmpc_set_latency_mapping_max_batch do not touch it.  Not combinable with block or band costs (their entry points take no
 * bmpc_cone_t).  bmpc_kinodyn_solve_batch_device keeps the reference's projection; bmpc_kinodyn_solve_batch_cone_device takes a bmpc_cone_t. */
typedef struct {
    int projection;                        /* 0: the reference's "SoC" step, 1: Euclidean */
    const double *mu; long smu;            /* [.][n_col][n_eff], NULL: bmpc_batch_t's scalar mu */
} bmpc_cone_t;
int bmpc_cone_struct_size(void);             /* sizeof(bmpc_cone_t), to catch binding drift */
int bmpc_biconvex_solve_batch_cone_device(const bmpc_batch_t *d, const bmpc_cone_t *c, void *hip_stream);
int bmpc_biconvex_solve_batch_cone_host(const bmpc_batch_t *d, const bmpc_cone_t *c);
/* The handle's projection (0 / 1) and per-foot coefficients mu [n_col][n_eff] (NULL: back to the scalar of
 * bmpc_biconvex_set_friction_coefficient); both persist across optimize calls.  optimize refuses (BMPC_BAD_ARG) projection 1 on a
 * handle that carries block or band costs or has n_col + 1 > 64, and a coefficient array under projection 0.  A KinoDynMP's
 * centroidal handle (bmpc_kinodyn_return_dyn) is solved through bmpc_biconvex_optimize: bmpc_kinodyn_optimize honours both settings
 * or returns that refusal. */
int bmpc_biconvex_set_cone_projection(bmpc_biconvex_t *h, int projection);
int bmpc_biconvex_set_friction_coefficients(bmpc_biconvex_t *h, const double *mu);
/* The largest scratch (private-segment) bytes per lane over the cone-projection kernels of one foot count (n_eff 2 or 4), as the
 * loaded code object reports them; -1 for another n_eff, or on error. */
int bmpc_biconvex_cone_kernel_scratch_bytes(int n_eff);

/* Friction cones about per-contact surface normals (additive, opt-in; with projection = 1 only) -----------------------------------
 * The Euclidean projection above has world z for its axis: flat ground.  With a unit normal n per problem, knot and foot (world
 * frame) the cone is |f - (n.f) n| <= mu n.f -- a slope, a stair edge, a tilted stepping stone.  The cone is rotationally symmetric,
 * so the normal is all the projection needs: with fn = n.f, ft = f - fn n, s2 = |ft|^2 of the gradient step f
 *     fn <= 0 and mu^2 s2 <= fn^2   -> (0, 0, 0)          (the polar cone; wins at the origin)
 *     fn >= 0 and s2 <= mu^2 fn^2   -> f, its bits unchanged
 *     otherwise                     -> s = sqrt(s2), t = (mu s + fn) / (mu^2 + 1), k = mu t / s: k ft + t n
 * With n = (0, 0, 1) these are the values of the projection above (only the sign of a zero can differ).  Everything else of the solve
 * is unchanged.  The kernels do not normalise.
 * normals: [.][n_col][n_eff][3]; each component finite and |n.n - 1| <= 1e-9 (the host entry point and the handle's setters check
 * that, the device entry point cannot).  snormals: batch stride in doubles, 0 = one set shared by the batch, otherwise at least
 * 3 * n_col * n_eff and at most 2^26.
 * fr == NULL, or fr->normals == NULL, is bmpc_biconvex_solve_batch_cone_device / _host itself: same kernel, same bits.  With normals
 * the batch runs "biconvex_admm_conef_kernel", chosen exactly as the cone kernel is (16 / 21 / 32 / 64 lanes per problem, one wave per
 * SIMD, both forms, every step tested on fp64 sums).  BMPC_BAD_ARG with a message naming the limit: normals under projection == 0,
 * fp32, n_col + 1 > 64 knots, n_eff other than 2 or 4, a stride outside the rule above, and (host entry point, setters) a normal that
 * is not finite or not of unit length.  Not built: normals in fp32, for more than 63 knots, and
 * for the reference's "SoC" step, which stays the reference's. */
typedef struct {
    const double *normals; long snormals;  /* [.][n_col][n_eff][3], unit, world frame; NULL: world z */
} bmpc_contact_frame_t;
int bmpc_contact_frame_struct_size(void);    /* sizeof(bmpc_contact_frame_t), to catch binding drift */
int bmpc_biconvex_solve_batch_cone_frames_device(const bmpc_batch_t *d, const bmpc_cone_t *c, const bmpc_contact_frame_t *fr, void *hip_stream);
int bmpc_biconvex_solve_batch_cone_frames_host(const bmpc_batch_t *d, const bmpc_cone_t *c, const bmpc_contact_frame_t *fr);
/* The handle's contact normals n [n_col][n_eff][3] (NULL: back to world z); they persist across optimize calls.  optimize refuses
 * (BMPC_BAD_ARG) normals under projection 0 and, as with projection 1 itself, on a handle that carries block or band costs or has
 * n_col + 1 > 64.  bmpc_kinodyn_optimize goes through the handle's optimize: it honours them or returns that refusal. */
int bmpc_biconvex_set_contact_normals(bmpc_biconvex_t *h, const double *n);
/* ... taken from the matrices of bmpc_biconvex_set_rotation_matrix_f: the normal of a contact is the third row of its R (row-major;
 * the reference's commented line is rotated_force = R * f, so local z is row 2 of R).  Refuses (BMPC_BAD_ARG) unless exactly
 * n_col * n_eff matrices were appended, knot-major, and every third row passes the unit test above.  The matrices themselves stay
 * stored and otherwise unused. */
int bmpc_biconvex_set_contact_normals_from_rotations(bmpc_biconvex_t *h);
/* The largest scratch (private-segment) bytes per lane over the kernels about contact normals of one foot count (n_eff 2 or 4), as the
 * loaded code object reports them; -1 for another n_eff, or on error. */
int bmpc_biconvex_cone_frame_kernel_scratch_bytes(int n_eff);

/* rigid-body model -------------------------------------------------------------------
 * What pinocchio::urdf::buildModel(urdf, JointModelFreeFlyer()) yields (inverse_kinematics.cpp:10,
 * kino_dyn.cpp:9), as flat arrays (the Python shim parses the URDF: bunmpc_amd/urdf_model.py).
 * nj must be 12 (free-flyer + serial chains numbered contiguously, parents first).
 * R [nj][9], p [nj][3]: joint placement in the parent joint frame; axis [nj][3];
 * bodies 0..nj (0 = base): mass, com [.][3], inertia about the com [.][9] (joint frame);
 * frames: body index + position in that body's joint frame. */
typedef struct bmpc_model bmpc_model_t;
bmpc_model_t *bmpc_model_create(int nj, const int *parent, const double *R, const double *p, const double *axis,
                                const double *mass, const double *com, const double *inertia, int nframes,
                                const int *frame_body, const double *frame_p);
void bmpc_model_destroy(bmpc_model_t *m);
double bmpc_model_total_mass(const bmpc_model_t *m);

/* inverse_kinematics_cpp.InverseKinematics -------------------------------------------
 * srcpy/ik/inverse_kinematics.cpp:20-39 over src/ik/{inverse_kinematics,com_tasks,end_effector_tasks,
 * regularization_costs}.cpp.  x = [q(19), v(18)], u = accelerations (18); frame = index into the
 * model's frame list.  Costs accumulate per node until optimize() and are then discarded. */
typedef struct bmpc_ik bmpc_ik_t;
bmpc_ik_t *bmpc_ik_create(const bmpc_model_t *model, int n_col);                                   /* :21 */
void bmpc_ik_destroy(bmpc_ik_t *h);
int bmpc_ik_n_col(const bmpc_ik_t *h);
int bmpc_ik_setup_costs(bmpc_ik_t *h, const double *dt, int n);                                     /* :22 */
int bmpc_ik_optimize(bmpc_ik_t *h, const double *x0);                                               /* :23 */
int bmpc_ik_get_xs(const bmpc_ik_t *h, double *xs);          /* (n_col+1) x 37                        :24 */
int bmpc_ik_get_us(const bmpc_ik_t *h, double *us);          /* n_col x 18                            :25 */
int bmpc_ik_return_opt_com(bmpc_ik_t *h, double *com);       /* (n_col+1) x 3                         :26 */
int bmpc_ik_return_opt_mom(bmpc_ik_t *h, double *mom);       /* (n_col+1) x 6                         :27 */
int bmpc_ik_add_position_tracking_task(bmpc_ik_t *h, int frame, int sn, int en, const double *traj3,
                                       double wt, const char *name);                               /* :29 */
int bmpc_ik_add_position_tracking_task_single(bmpc_ik_t *h, int frame, const double *traj3, double wt,
                                              const char *name, int time_step);                    /* :30 */
int bmpc_ik_add_terminal_position_tracking_task(bmpc_ik_t *h, int frame, const double *traj3, double wt,
                                                const char *name);                                 /* :31 */
int bmpc_ik_add_velocity_tracking_task(bmpc_ik_t *h);        /* prints "function not implemented"     :32 */
int bmpc_ik_add_com_position_tracking_task(bmpc_ik_t *h, int sn, int en, const double *traj, int rows,
                                           double wt, const char *name, int is_terminal);          /* :33 */
int bmpc_ik_add_centroidal_momentum_tracking_task(bmpc_ik_t *h, int sn, int en, const double *traj, int rows,
                                                  double wt, const char *name, int is_terminal);   /* :34 */
int bmpc_ik_add_state_regularization_cost(bmpc_ik_t *h, int sn, int en, double wt, const char *name,
                                          const double *w36, const double *xreg37, int is_terminal); /* :35 */
int bmpc_ik_add_state_regularization_cost_single(bmpc_ik_t *h, int time_step, double wt, const char *name,
                                                 const double *w36, const double *xreg37);        /* :36 */
int bmpc_ik_add_ctrl_regularization_cost(bmpc_ik_t *h, int sn, int en, double wt, const char *name,
                                         const double *w18, const double *ureg18, int is_terminal); /* :37 */
int bmpc_ik_add_ctrl_regularization_cost_single(bmpc_ik_t *h, int time_step, double wt, const char *name,
                                                const double *w18, const double *ureg18);         /* :38 */
/* additive: DDP telemetry of the last optimize; status 0 converged, 1 maxiter, 2 regularisation maxed */
int bmpc_ik_last_stats(const bmpc_ik_t *h, int *iters, int *status, double *cost, double *stop);

/* batch of independent IK problems (additive).  Device pointers:
 *   x0 [B][37], dt [B][n_col], tasks [B][n_col+1][BMPC_IK_NODE_TASK_DOUBLES] per node:
 *       4 x {weight, frame, ref(3)} | com {weight, ref(3)} | mom {weight, ref(6)} | state weight | ctrl weight
 *   state_w [.][36], ctrl_w [.][18] (batch stride 0 = shared), x_reg [B][37]; with node strides sn_* != 0 these are per
 *       node too: state_w [.][n_col+1][36], x_reg [.][n_col+1][37] (batch stride s_x_reg, 0 = 37), ctrl_w [.][n_col][18]
 *       (what the acyclic generator's time-varying add_*_regularization_cost_single calls produce)
 *   ws [B][bmpc_ik_workspace_doubles(n_col)] scratch + results (offsets: bmpc_ik_layout), active: one int */
#define BMPC_IK_NODE_TASK_DOUBLES 33
/* Scheduling thresholds of ONE batch solve (no effect on results; they replace flipping the process-wide bmpc_ik_set_* defaults
 * around a call, which raced between host threads driving different streams).  Every field: 0 = the process default,
 * < 0 = never, n > 0 = while at most n problems are still iterating.
 * ABI version 2 (bmpc_abi_version): bmpc_ik_batch_t ends in this struct and active_list grew with it.  A caller MUST
 * zero-initialise the whole bmpc_ik_batch_t (memset) before filling it -- a zero sched is "all defaults, no test switch" --,
 * check bmpc_ik_batch_struct_size() == sizeof(bmpc_ik_batch_t), and size active_list with bmpc_ik_active_list_ints(B), never with
 * a formula of its own (the list code writes the express lane's xlist / xmeta behind the two lists). */
typedef struct {
    int spec_below;         /* four step lengths of a problem side by side (bmpc_ik_set_speculative_below) */
    int all_steps_below;    /* all ten step lengths at once on three workgroups (bmpc_ik_set_all_steps) */
    int gains_wave_below;   /* a second wave per problem for the Riccati gains (bmpc_ik_set_gains_wave_below) */
    int express_cap;        /* NOT a threshold: the most problems the express lane may take off the batch (bmpc_ik_set_express_capacity;
                               0 = the process default, < 0 = no express lane) */
    int debug_inject;       /* tests only: 1 = overwrite the first active-list entry with an out-of-range index right after the
                               list is initialised; the solve must then return BMPC_DEVICE_ERROR (index checks of the list code);
                               2 = the express lane takes its problems in front of iteration 2 whatever the batch looks like;
                               any other value is ignored (as 0) */
} bmpc_ik_sched_t;
typedef struct {
    int B, n_col, maxiter;
    const bmpc_model_t *model;
    const double *x0, *dt, *tasks, *state_w, *x_reg, *ctrl_w;
    long s_state_w, s_ctrl_w;
    double *ws;
    int *active;
    int *iters_run;   /* host int or NULL: DDP iterations the loop executed */
    long s_x_reg, sn_state_w, sn_x_reg, sn_ctrl_w;   /* 0 = defaults: x_reg [B][37], one vector per problem */
    int *active_list; /* device, bmpc_ik_active_list_ints(B) ints of scratch, or NULL.  With it every launch of the DDP loop covers
                         only the problems still iterating (an index list the forward pass rebuilds each iteration), and the few
                         problems whose line search goes past four step lengths get all ten at once from then on; without it
                         every launch covers all B and finished problems return at once.  Results do not depend on it. */
    bmpc_ik_sched_t sched;
} bmpc_ik_batch_t;
int bmpc_ik_batch_struct_size(void);     /* sizeof(bmpc_ik_batch_t), to catch binding drift */
/* diagnostics: workgroups of each IK kernel a CU holds at once according to the runtime's occupancy query, in the order calcdiff
 * (two waves per node pair), calcdiff1 (one wave per pair), backward<1>, backward<2>, forward<1>, forward<2>, forward<3>, state */
void bmpc_ik_kernel_occupancy(int *out8);
long bmpc_ik_active_list_ints(long B);   /* length of bmpc_ik_batch_t.active_list */
int bmpc_ik_workspace_doubles(int n_col);
void bmpc_ik_layout(int n_col, long *offsets8);      /* xs, us, scalars, K, k, fs, Lx, Lqq (the q-block of L_xx in MFMA tile layout) */
/* telemetry: rows [iteration i < *iters][*width = 4] at *offset of a problem's workspace: cost, regularisation, accepted step
 * length (0 = none) and stopping criterion |Q_u|^2 as SolverDDP holds them at the end of iteration i */
void bmpc_ik_layout_trace(int n_col, long *offset, int *iters, int *width);
/* Line-search scheduling of the batched DDP (no effect on results): while at most n_active problems are still
 * iterating, four step lengths of a problem are tried side by side (one wave per problem) instead of one after the
 * other (four problems per wave); with at most bmpc_ik_set_all_steps' n_active left (default 0 = never: no measurable gain, EXPERIMENTS.md 9), all ten step
 * lengths at once on three workgroups per problem.  Default 1024 (one wave per SIMD of an MI355X); 0 = never.  Both return
 * the old value. */
int bmpc_ik_set_speculative_below(int n_active);
/* (experiment switch) with MORE than n_active problems iterating -- and at most the bound above -- the side-by-side line search runs
 * every role of a problem on ONE wave instead of two (as many waves as problems: one round over the chip's SIMDs where two waves per
 * problem need two).  Default 0 = never.  Returns the old value. */
int bmpc_ik_set_spec_one_wave_above(int n_active);
int bmpc_ik_set_all_steps(int n_active);
/* Riccati-pass scheduling (no effect on results): while at most n_active problems are still iterating, each gets a second
 * wave that computes and stores the gains K, k one node behind the recursion.  Default 512; 0 = never.  Returns the old value. */
int bmpc_ik_set_gains_wave_below(int n_active);
/* Host waits of the DDP loop (no effect on results): 1 (default) = the waiting host thread sleeps until the device's interrupt
 * (hipEventBlockingSync), 0 = it spins.  Returns the old value. */
int bmpc_ik_set_blocking_waits(int on);
/* The express lane (needs bmpc_ik_batch_t.active_list; no effect on results).  A batch that converges fast leaves a thin tail of
 * problems iterating long after the rest has finished, and in lock-step those pay every early iteration at the whole batch's pace.
 * In front of iterations 2..12 a one-workgroup kernel looks at the batch and, ONCE -- when (almost) nobody has finished yet, at
 * least half of the problems are near the stopping threshold and an iteration earlier (almost) none was -- takes the n problems
 * farthest from it (never more than an eighth of the batch) off the active list; a persistent fused kernel (one four-wave
 * workgroup per problem: derivative pass, Riccati pass and line search of whole DDP iterations without leaving the chip, no
 * host look) runs them to the end on a side stream while the batch goes on without them.  Default 96; 0 = no express lane.
 * Returns the old value. */
int bmpc_ik_set_express_capacity(int n);
/* Batches of at most n problems (the single-problem handles InverseKinematics / KinoDynMP above all) run their whole DDP in ONE
 * launch of the fused kernel, every problem on a CU of its own, with no host look between iterations (no effect on results).
 * Default 16; 0 = never.  Returns the old value. */
int bmpc_ik_set_fused_direct_max(int n);
/* ... and what "near the stopping threshold" means in that trigger: |Q_u|^2 < stop at the problem's last Riccati pass (SolverDDP
 * stops below 1e-9).  Default 1.0.  Returns the old value. */
double bmpc_ik_set_express_near(double stop);
int bmpc_ik_solve_batch_device(const bmpc_ik_batch_t *d, void *hip_stream);
/* Measurement aid (additive): with profiling on, the DDP loop brackets each of its kernels with events; after a batch solve
 * bmpc_ik_last_profile returns the summed milliseconds of ik_state / ik_calcdiff / ik_backward / ik_forward and of the rest
 * of the loop (bench.py's per-kernel split; rocprofv3 --kernel-trace gives the same numbers, profiles/). */
/* self test (host arrays): the state operators diff(x0, x1) and x0 (+) dx of n samples, x [n][37], dx [n][36], by the
 * quaternion versions the forward pass uses (dq [n][36], iq [n][37]) and by the rotation-matrix versions (dr, ir) */
int bmpc_ik_selftest_state_ops(const double *x0, const double *x1, const double *dx, int n, double *dq, double *dr, double *iq, double *ir);
/* TEST ONLY.  Self test of the derivative pass and the Riccati pass, each launched ONCE at a trajectory of the caller's (device
 * arrays xs [B][n_col+1][37], us [B][n_col][18]; d as for bmpc_ik_solve_batch_device, maxiter / iters_run / sched ignored): the
 * workspace is initialised as a solve does, its rows xs / us and the scalars feasible (is_feasible_; was_feasible_ = 0) and xreg
 * (= ureg, in [1e-9, 1e9)) are overwritten, then the DDP loop's own launchers run the state kernel, the derivative kernel
 * (calcdiff_kernel: 0 = two waves per node pair, 1 = one wave per pair, whatever the launch's size) and the backward kernel
 * (bwd_waves: 1, or 2 = with the gains wave).  No forward pass, no host loop; returns after the stream has drained, the results
 * are in d->ws (bmpc_ik_layout_all); the node costs, which the Riccati pass sums and then overwrites, are kept in the solver's
 * unused Quuk rows, node t at Quuk[t].  Bad arguments: BMPC_BAD_ARG. */
int bmpc_ik_selftest_passes(const bmpc_ik_batch_t *d, const double *xs, const double *us, int feasible, double xreg, int calcdiff_kernel,
                            int bwd_waves, void *hip_stream);
/* TEST ONLY.  Offsets (doubles) into a problem's workspace, the first min(n, count) of: xs, us, scalars, K, k, fs, Lx, Lqq (as
 * bmpc_ik_layout), xnext, Hn (momentum Jacobian, its weight and the velocity diagonal of L_xx), Lu, Luu (diagonal), A6, B6 (the
 * 6 x 6 Jintegrate blocks), nrs, njl, ncs (state residual, its Jlog6 block transposed, state + control cost of a node), total,
 * Quuk (unused by the solver; bmpc_ik_selftest_passes keeps the node costs there).  Returns count (19). */
int bmpc_ik_layout_all(int n_col, long *offsets, int n);
/* Derivative-pass scheduling (no effect on results): a launch with MORE than n_pairs node pairs (active problems x ceil((n_col + 1)
 * / 2)) runs one wave per pair instead of two.  Default 1024 (what an MI355X holds of the two-wave kernel); returns the old value.
 * bmpc_ik_last_calcdiff_kernel: which kernel the last derivative launch of this process was (0 two waves, 1 one wave, -1 none yet). */
int bmpc_ik_set_calcdiff_one_wave_above(int n_pairs);
int bmpc_ik_last_calcdiff_kernel(void);
/* TEST ONLY.  What the DDP loop of a batch of B problems and n_col running nodes would launch at a host look that finds `active`
 * problems (1 .. B) still iterating, under the process's current bmpc_ik_set_* defaults and `sched` (NULL: none; fields as in
 * bmpc_ik_batch_t.sched): the loop's own plan functions (bunmpc_amd/csrc/ik_plan.h), which make no GPU call -- this runs on a machine
 * without one.  has_list / has_wide: the batch has an active_list (both 1) or none (both 0).  Batch level: fused_direct (the whole
 * solve is one launch of ik_fused_kernel, of fused_grid workgroups; the rest of the plan then does not run), express_cap (what the
 * express lane may take, 0 = no lane; its ik_fused_kernel has express_grid workgroups).  Look level: chunk (DDP iterations enqueued
 * before the next look), fwd_map (0 four problems per wave, 1 / 2 / 3 four step lengths at once on one / two / three waves, 4 all ten
 * on three workgroups), bwd_waves, n_launch, and kernel name, workgroups and workgroup size of the four launches of an iteration.
 * The constants: the longest horizon of the fused kernel, the iterations in front of which the express lane looks, the chunk length
 * once the line search is no longer sequential.  status: BMPC_OK, or BMPC_BAD_ARG (also returned) for sizes out of range. */
typedef struct { char kernel[24]; unsigned grid, block; } bmpc_ik_planned_launch_t;
typedef struct {
    int status;
    int fused_direct, express_cap;
    unsigned fused_grid, express_grid;
    int chunk, fwd_map, bwd_waves, n_launch;
    bmpc_ik_planned_launch_t state, calcdiff, backward, forward;
    int max_fused_col, express_first_iter, express_last_iter, tail_chunk;
} bmpc_ik_iter_plan_t;
int bmpc_ik_plan_iteration(int B, int n_col, int maxiter, int has_list, int has_wide, int active, const bmpc_ik_sched_t *sched,
                           bmpc_ik_iter_plan_t *out);
int bmpc_ik_set_profile(int on);            /* returns the old setting */
void bmpc_ik_last_profile(double *ms5);
/* [com, vcom, hg.angular] of x = [q, v]: what KinoDynMP::optimize feeds the centroidal solve (kino_dyn.cpp:42,86-97) */
int bmpc_ik_centroidal_state_device(const bmpc_model_t *model, const double *x, double *out9, int B, void *hip_stream);

/* biconvex_mpc_cpp.KinoDynMP ---------------------------------------------------------
 * srcpy/motion_planner/biconvex.cpp:55-63 over src/motion_planner/kino_dyn.cpp */
typedef struct bmpc_kinodyn bmpc_kinodyn_t;
/* n_eff must be 4 here and in bmpc_kinodyn_solve_batch_device (BMPC_BAD_ARG otherwise): the IK model is a 12-joint quadruped */
bmpc_kinodyn_t *bmpc_kinodyn_create(const bmpc_model_t *model, double m, int n_eff, int dyn_col, int ik_col); /* :56 */
void bmpc_kinodyn_destroy(bmpc_kinodyn_t *h);
bmpc_biconvex_t *bmpc_kinodyn_return_dyn(bmpc_kinodyn_t *h);      /* borrowed, owned by h           :57 */
bmpc_ik_t *bmpc_kinodyn_return_ik(bmpc_kinodyn_t *h);             /* borrowed, owned by h           :58 */
int bmpc_kinodyn_optimize(bmpc_kinodyn_t *h, const double *q, const double *v, int dyn_iters, int kino_dyn_iters); /* :59 */
int bmpc_kinodyn_set_com_tracking_weight(bmpc_kinodyn_t *h, double w);                              /* :60 */
int bmpc_kinodyn_set_mom_tracking_weight(bmpc_kinodyn_t *h, double w);                              /* :61 */
int bmpc_kinodyn_compute_solve_times(bmpc_kinodyn_t *h);                                            /* :62 */
int bmpc_kinodyn_return_solve_times(const bmpc_kinodyn_t *h, double *t3);  /* dyn, ik, total seconds  :63 */

/* batch of KinoDynMP::optimize calls (additive), all pointers on the device:
 *   x [B][37] = [q, v];  dyn.x_init [B][9] is OVERWRITTEN with [com, vcom, hg.angular] of x (kino_dyn.cpp:42),
 *   dyn solved (use cold_start = 1 for set_warm_starts' behaviour), then the com / momentum
 *   references of ik.tasks are OVERWRITTEN from dyn.X (kino_dyn.cpp:50-56; their weights are the
 *   caller's wt_com / wt_mom already in the task blocks) and the IK-DDP runs. */
typedef struct {
    bmpc_batch_t dyn;
    bmpc_ik_batch_t ik;
    const double *x;
} bmpc_kinodyn_batch_t;
int bmpc_kinodyn_solve_batch_device(const bmpc_kinodyn_batch_t *d, void *hip_stream);
/* The same with the centroidal stage through bmpc_biconvex_solve_batch_cone_device or, with frames, ..._cone_frames_device: the
 * Euclidean cone projection, per-foot coefficients and contact normals (bmpc_cone_t, bmpc_contact_frame_t above) in the whole-body
 * data path.  Their refusals (returned before anything is written or launched) and their kernels.  cone == NULL is
 * bmpc_kinodyn_solve_batch_device itself, bit for bit; frames may be NULL. */
int bmpc_kinodyn_solve_batch_cone_device(const bmpc_kinodyn_batch_t *d, const bmpc_cone_t *cone, const bmpc_contact_frame_t *frames, void *hip_stream);

/* harness inputs on the device (additive; SURVEY 8f-1, centroidal level) -----------------------------
 * What SoloMpcGaitGen.create_cnt_plan / create_costs compute per MPC call (abstract_cyclic_gen.py:159-414, 564-607)
 * for B problems at once, data path only (no MCTS locations or noise; flat ground -- bmpc_plan_batch_terrain_device takes a height
 * map): from the current CoM, foot
 * positions, time, desired velocities -> cnt_plan [B][H][4][4], swing_time [B][H][4], dt [B][H], X_nom [B][9H],
 * X_ter [B][9], ready to be handed to bmpc_biconvex_solve_batch_device without leaving HBM.  The gait table is
 * DEVICE memory as well (n_gaits entries; gait_id [B] selects, NULL = entry 0). */
typedef struct {
    double gait_period, gait_dt, gait_horizon, nom_ht;
    double stance_percent[4], phase_offset[4];
    double ori_correction[3];
    double offsets_xy[4][2];     /* hip offsets from the CoM after the harness' rounding and +-0.04 widening (:56-72) */
} bmpc_gait_params_t;
typedef struct {
    int B, n_col, n_gaits, reserved_;
    const bmpc_gait_params_t *gaits;   /* device */
    const int *gait_id;                /* [B] or NULL */
    const double *t0;                  /* [B] */
    const double *com;                 /* [B][3] centre of mass (xy are rounded to 3 decimals inside, :164) */
    const double *feet0;               /* [B][4][3] current foot positions (rounded inside, :215) */
    const double *v_des;               /* [B][3] desired CoM velocity, already in the yaw frame */
    const double *w_des;               /* [B] */
    const double *x_init;              /* [B][9] centroidal state */
    const double *amom;                /* [B][3] orientation-correction momentum (:616-627) or NULL */
    const double *hip_off;             /* [B][4][2] yaw-rotated hip offsets or NULL (gaits[].offsets_xy) */
    double *cnt_plan, *swing_time, *dt, *X_nom, *X_ter;
} bmpc_plan_batch_t;
int bmpc_plan_batch_device(const bmpc_plan_batch_t *d, void *hip_stream);

/* The same for whole-body states: everything SoloMpcGaitGen.optimize prepares before kd.optimize
 * (abstract_cyclic_gen.py:629-663 -> create_cnt_plan, create_costs) from x = [q, v], the time and the desired body-frame
 * velocity, on the device: forward kinematics (CoM, feet, centroidal state), v_des in the world frame, yaw-rotated hip
 * offsets, the orientation-correction momentum log3(R_q^T), then the contact plan / cost references as above and the
 * IK task blocks of bmpc_ik_batch_t (frame tasks from the plan; CoM / momentum weights, their references are filled
 * by bmpc_kinodyn_solve_batch_device).  w_des = 0 (the data path).  Outputs feed bmpc_kinodyn_solve_batch_device. */
typedef struct {
    int B, n_col, ik_col, reserved_;
    const bmpc_model_t *model;
    const bmpc_gait_params_t *gait;    /* device, one entry; offsets_xy in the body frame */
    int foot_frame[4];                 /* frame indices of the end effectors (eff_names) */
    double step_ht, swing_wt[2], cent_wt[2], reg_wt[2];   /* weight_abstract.py fields the task list uses */
    const double *x;                   /* [B][37] */
    const double *t0;                  /* [B] */
    const double *v_des_body;          /* [B][3] */
    /* intermediates (device, caller-allocated): */
    double *com, *feet0, *v_des, *w_des, *hip_off, *amom;   /* [B][3], [B][4][3], [B][3], [B], [B][4][2], [B][3] */
    /* outputs: */
    double *x_init;                    /* [B][9] centroidal state of x */
    double *cnt_plan, *swing_time, *dt, *X_nom, *X_ter;
    double *ik_tasks;                  /* [B][ik_col + 1][33] */
} bmpc_wb_plan_batch_t;
int bmpc_wb_plan_batch_device(const bmpc_wb_plan_batch_t *d, void *hip_stream);

/* Both plans on a terrain height map (additive): what the reference's harness does with its `height_map` argument
 * (abstract_cyclic_gen.py:333-337, 370-374).  A new stance location and every swing location get z = height(x, y) + foot size; knot 0
 * stays the current feet and a continuing stance copies the previous knot.  The via-point height step_ht, nom_ht in X_nom / X_ter and
 * the IK task layout stay absolute, as in the reference.  normals [B][n_col][4][3] (device, or NULL: not wanted) receives the unit
 * normal of the terrain under every knot's (x, y): what bmpc_contact_frame_t takes, without leaving HBM.
 * The map: heights [.][ny][nx] (device), node (iy, ix) at (x0 + ix cell, y0 + iy cell), bilinear in between, the border's height
 * outside; sheights = doubles between the problems' maps, 0 = one map for the batch.  With u = (x - x0) / cell and v likewise, both
 * clamped to the map BEFORE the conversion to an index (so no x, y, finite or not, reads outside it), ix = min(floor(u), nx - 2),
 * a = u - ix, b = v - iy:   d0 = z10 - z00, d1 = z11 - z01, h0 = z00 + a d0, h1 = z01 + a d1, h = h0 + b (h1 - h0),
 * gx = (d0 + b (d1 - d0)) / cell, gy = (h1 - h0) / cell, r = sqrt((gx gx + gy gy) + 1), n = (-gx, -gy, 1) / r -- separate multiplies
 * and adds, the arithmetic of bunmpc_amd/terrain.py.
 * BMPC_BAD_ARG with a message naming the limit: a NULL t or NULL heights, nx or ny outside [2, 4096], cell not finite and > 0, x0 / y0
 * not finite, sheights neither 0 nor in [nx * ny, 2^26], and everything the plain calls refuse.  The heights are device memory: they
 * are not checked (a NaN height gives NaN heights and normals, never a read outside the map). */
typedef struct {
    int nx, ny;
    double x0, y0, cell;
    const double *heights;   /* device, [.][ny][nx] */
    long sheights;           /* doubles between problems' maps; 0 = one map for the batch */
} bmpc_terrain_t;
int bmpc_terrain_struct_size(void);          /* sizeof(bmpc_terrain_t), to catch binding drift */
int bmpc_plan_batch_terrain_device(const bmpc_plan_batch_t *d, const bmpc_terrain_t *t, double *normals, void *hip_stream);
int bmpc_wb_plan_batch_terrain_device(const bmpc_wb_plan_batch_t *d, const bmpc_terrain_t *t, double *normals, void *hip_stream);

/* The 1 kHz plan of SoloMpcGaitGen.optimize (abstract_cyclic_gen.py:677-692) for a batch, on the device:
 * out[b] = vstack_{i < size} linspace(knots[b][i], knots[b][i+1], int(dt[b][i] / step)), end points included (and so
 * repeated at the seams, as there).  knots [B][n_knots][width], dt [B][dt_stride] (first `size` entries used),
 * out [B][max_rows][width], rows [B] = number of rows written for each problem (<= max_rows; more are dropped). */
typedef struct {
    int B, n_knots, width, size, max_rows, dt_stride;
    double step;
    const double *knots, *dt;
    double *out;
    int *rows;
} bmpc_interp_batch_t;
int bmpc_interp_batch_device(const bmpc_interp_batch_t *d, void *hip_stream);

/* Output stage of the data path: InverseDynamicsController.id_joint_torques
 * (ISL/examples/controllers/robot_id_controller.py:57-86) and the rows the rollout loop records from it
 * (ISL/examples/iterative_algorithm/simulation.py:484-528), for n samples at once, on the device:
 *   tau_ff = (rnea(q_des, v_des, a_des) - sum_j J_j(q_des)^T [f_j; 0])[6:]
 *   tau_fb = -kp (q[7:] - q_des[7:]) - kd (v[6:] - v_des[6:])
 *   action = (tau_ff + tau_fb + kd v[6:]) / kp + q[7:]                     (action_type "pd_target")
 *   state  = [v (18) | q[0:2] - foot_j[0:2], j < 4 (8) | q[2:] (17)]        (43 doubles)
 * Every input is a device array of rows with its own row stride in doubles, so the rows of the 1 kHz plan
 * (xs_int: q at +0, v at +19, stride 37; us_int; f_int) can be passed in place.  q / v NULL = the desired rows
 * (a sample exactly on its plan: tau_fb = 0).  Outputs are dense ([n][12], [n][43]); NULL ones are skipped.
 * Each end effector must hang off a different leg. */
typedef struct {
    long n;
    const bmpc_model_t *model;
    int foot_frame[4];                 /* frame indices of the end effectors, in the order of f */
    double kp[12], kd[12];
    const double *q, *v;               /* measured state: rows of 19 / 18 */
    const double *q_des, *v_des, *a_des, *f;   /* rows of 19 / 18 / 18 / 12 */
    long s_q, s_v, s_q_des, s_v_des, s_a_des, s_f;
    double *tau_ff, *tau_fb, *action, *state;
} bmpc_id_batch_t;
int bmpc_id_batch_device(const bmpc_id_batch_t *d, void *hip_stream);

/* Contact-conditioned perturbation of nominal states: the sampler of the data-collection loop
 * (ISL/examples/iterative_algorithm/data_collection.py:188-262) for B nominal states at once, on the device.
 * For state b the draws z[b][0..K) (standard normal, 36 each: 18 for the position, 18 for the velocity perturbation)
 * are consumed in order until one gives a configuration with no foot below the ground, as the reference's while loop
 * does: pos = mu + sigma z (mu / sigma = base position, base orientation, joint position, velocity),
 * q' = integrate(q, (I - pinv(J) J) pos), v' = v + (I - pinv(J * vel) (J * vel)) pos with J the stacked linear
 * Jacobians of the feet whose contact flag is 1.  chosen[b] = index of the accepted draw, or -1 when all K were
 * rejected (q_out / v_out then hold the nominal state and the caller draws again for that state).
 * contact: flag of foot e of state b at contact[b * s_contact_b + e * s_contact_e], so a contact-plan row
 * (cnt_plan[b][knot][e][0]) can be passed in place. */
typedef struct {
    int B, K;
    const bmpc_model_t *model;
    int foot_frame[4];
    double mu[4], sigma[4];
    const double *q, *v;               /* [B][19], [B][18] nominal states */
    const double *contact;
    long s_contact_b, s_contact_e;
    const double *z;                   /* [B][K][36] */
    double *q_out, *v_out;             /* [B][19], [B][18] */
    int *chosen;                       /* [B] */
} bmpc_perturb_batch_t;
int bmpc_perturb_batch_device(const bmpc_perturb_batch_t *d, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
