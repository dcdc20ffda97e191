// The body of the batched centroidal ADMM kernel (one knot per lane): template admm_body<AdmmCfg<R, LPP, E, RAW, HASQF, ...>>.  Included inside
// the anonymous namespace of biconvex_admm.hip, which is compiled once per unit (the fp32 units with other compiler flags: see
// bunmpc_amd/build.py); the mapping, the reference lines and the algebra are described at the top of biconvex_admm.hip.
#pragma once

// ------------------------------------------------------------------------------
// Per-iteration algebra (what differs from the reference's formulation, all of it exact
// algebra on the same quadratic):
//   * acceptance test.  fista.cpp:16 tests  f(y+) - f(y) > g.d + (L/2)|d|^2 ; for the quadratic
//     f = y'Qy + q'y + rho|Ay - b + P|^2 that difference is  g.d + d'Qd + rho|A d|^2  identically,
//     and A d = (A y+ + bPk) - (A y + bPk) is at hand, so the test becomes
//     d'Qd + rho|A d|^2 > (L/2)|d|^2 : two segment sums instead of three, no cancellation.
//   * x_init rows.  A_f's last nine rows are the identity on X_0 (centroidal.hpp:22-27), i.e. the
//     term rho|X_0 - x_init + P_H|^2: a diagonal quadratic in X_0.  Lane 0 adds rho to its Q and
//     2 rho (P_H - x_init) to its q instead of every lane carrying nine extra residual rows.
//   * momentum coefficients (t_k - 1)/t_{k+1} (fista.cpp:34-35) depend on the iteration index
//     only: one table per device (biconvex_launch.hip: momentum_table), read by scalar loads.
//   * a problem that finishes (|d| < tol or maxit) has its iterate latched into `fin` registers
//     at that moment; the loop body itself carries no per-lane freeze selects.
//
// STEAL (round 4; LPP = 21, many ADMM iterations): the grid is what the chip holds at once and a SEGMENT whose problem has finished
// -- the ADMM's early exit (biconvex.cpp:111-114) makes the iteration counts differ per problem: 34 .. 100 at num_iters = 100 --
// stores its results and takes the next unsolved problem from a device counter, instead of idling until the slowest problem of its
// wave is done (a wave's time was the MAXIMUM over its three problems; the batch's now approaches the SUM over all problems / the
// number of segments).  The ITERATES of a problem do not depend on which segment runs it, or when: X, F, P, the step constants and every
// count are the same bits.  Its segment SUMS do: a 21-lane segment lies across the DPP rows 16|5, 11|10 or 6|15 by its position in the wave,
// so its terms are added in another order, within 2 gamma_6 of each other (gamma_6 = 6u / (1 - 6u), u = 2^-53) -- which shows in the reported
// violation and its history, and could flip a step decision whose sum lies within that of its threshold
// (tests/test_biconvex_gpu.py::test_result_does_not_depend_on_the_segment holds both; tests/test_lane_probe_gpu.py pins the three orders).
// Addresses in this mode are the arrays' own bases + 32-bit byte offsets from the problem index (the host checks that they fit).
//
// XLDS (round 4; the build for TWO waves per SIMD, 256 registers): the FISTA loops keep y and its image in registers only; x_k and
// ITS image rest in LDS (the problem's X / F block and an R block beside them).  An iteration reads them once -- while the segment
// sums of its step are being reduced -- for the momentum step, and leaves x_{k+1} there under the mask of the problems still
// iterating, which is also the latch of a finishing problem.  36 registers less across the loops than two register copies whose
// roles swap: both loops are free of scratch accesses at 256 registers.  Same operations in the same order: same bits.
//
// CLDS (a second build for two waves per SIMD: 32 lanes, four feet, harness form, fp64, 17 .. 21 knots): XLDS, except that in the two
// CERTIFIED loops it is 18 constants of the phase that rest in LDS -- read early, never written -- while x_k and its image stay in
// registers; the X / F / R blocks are written only when a problem finishes or hands over (see the motion step).  Same bits again.
//
// WAVES > 1 (round 4; horizons of 64 .. 255 knots: the reference's own sweep of solve times goes to 10 s horizons,
// examples/analysis/solve_times_test.py): ONE problem per WORKGROUP of WAVES wave64s, knot t on thread t.  The knot t <-> t +- 1
// exchanges cross the wave boundaries through LDS (lane 0 / lane 63 of every wave leave their values, one workgroup barrier, the
// neighbour wave's edge lane picks them up), the segment sums are the waves' sums added in wave order by every wave (same bits
// everywhere, so every decision stays workgroup-uniform and the barriers sit in uniform control flow); buffers alternate between
// two copies, so one barrier per exchange is enough.  Everything else is the one-wave code.
// Step certificate of the force step: margin eta of the test  bound <= (L/2)(1 - eta), and the factor of the
// |d|^2 floor below which the certified loop hands a step to the tested one: 2 (|a| + |b|)^2 <= 2|a|^2 + 2|b|^2, noise <= 2^-40 of
// the images' scale (2^-53: a few ulp per image, with room for the iterates to grow within the phase), (5 / eta)^2 from the margin's
// split.
constexpr double kCertEta = 1.0 / 64.0;
constexpr double kCertFloor = 2.0 * 25.0 / (kCertEta * kCertEta) * 0x1p-80;
// Stage 1 of the lane-local screen in the headline kernel's certified loops ("Two-stage screen"): the components of
// the lane's step whose squares are summed first -- the motion step's velocity z, the force step's fz of the third foot (one foot's fz
// settles 77-78 % of the trot batch's wave-iterations whichever foot it is).  Any subset is sound (see the force step); which one is a
// matter of speed alone, tuned on the trot batch with tools/screen_rate.py --terms.
// (Namespace scope: a constexpr array of admm_body indexed inside a lambda would be captured by its closure.)
[[maybe_unused]] constexpr int kScreenTermsX[] = {5};
[[maybe_unused]] constexpr int kScreenTermsF[] = {8};
// (wave, force phase) pairs that the loop-constants build ran two feet per lane, since the last reset (AdmmUnit::foot_pair_phases): one
// vector atomic of lane 0 per such phase, telemetry for the tests of the eligibility rule
[[maybe_unused]] __device__ unsigned long long g_foot_pair_phases = 0;

// MATES (a launch geometry of the loop-constants build: DESIGN.md section 9 item 4).  The two waves that share a SIMD do not share it
// evenly: at equal priority the older one issues nearly unimpeded, finishes early, and the younger runs its remainder alone at about
// two thirds of the pair's throughput (profiles/simd_mates_step0.txt).  With one-wave workgroups the mates are grid indices i and
// i + 1024 and cannot see each other; here a workgroup is EIGHT waves -- two per SIMD of its CU -- each with its own two problems,
// (block x 8 + wave) x 2 + segment, and its own LDS area of loop_constants_lds_bytes, and behind the eight areas a mailbox of 16 words:
// [0 .. 8) the SIMD a wave runs on (HW_REG_HW_ID, read once at entry; published in front of the kernel's one barrier), [8 .. 16) the
// phase a wave has entered, counted from 1 (0: none yet; kMateDone: its solve is over).  A wave's mate is the one other wave of the
// workgroup with its SIMD number; a wave that finds none, or several, takes no further part.  At the head of every force and motion
// phase a wave publishes its count n and reads its mate's m: m >= n and the mate still solving -- the mate is level or ahead -- it
// raises its priority (s_setprio 1), otherwise it lowers it (0).  Priority outranks age, so the wave behind takes the issue slots until
// it has caught up: a phase or two later the roles swap.  The mailbox decides priorities only -- stale or wrong words cost time, never a
// result -- and nothing is added inside the FISTA loops.  BatchArgs::force_foot_pairs carries the switch in bit 1 (bit 0: two feet per
// lane): off, the geometry runs without the rule (every wave at priority 0).
constexpr int kMateDone = 0x7fffffff;
template <bool MATES, typename A>
__device__ __forceinline__ constexpr decltype(auto) wave_lds(A &all, unsigned offset) {
    if constexpr (MATES) return static_cast<double *>(all + offset);
    else return (all);
}
#ifdef BMPC_SIMD_STAMPS
// The diagnostic build of tools/simd_mates_stamps.py alone (the shipped kernels execute no stamp): when a wave
// of the loop-constants build starts and ends and where it runs, 8 words per wave of BatchArgs::simd_stamps -- [0] the 100 MHz clock at
// entry, [1] HW_REG_HW_ID (register 4: wave slot, SIMD, CU, shader array and engine) | HW_REG_XCC_ID (register 20) << 32, [2] the
// shader clock at entry, [3] and [4] the two clocks at exit.  Written by lane 0 at once: nothing is held across the kernel, and no
// output is computed from a stamp.
__device__ __forceinline__ void simd_stamp(unsigned long long *stamps, bool entry) {
    if (!stamps) return;
    unsigned long long *w = stamps + 8 * ((size_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64);
    const unsigned long long rt = __builtin_amdgcn_s_memrealtime(), clk = __builtin_amdgcn_s_memtime();
    if ((threadIdx.x & 63) != 0) return;
    if (entry) {
        w[0] = rt;
        w[1] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | 31 << 11) | (unsigned long long)__builtin_amdgcn_s_getreg(20 | 31 << 11) << 32;
        w[2] = clk;
    } else {
        w[3] = rt;
        w[4] = clk;
    }
}
#endif

// BQ (per-knot block-diagonal costs: raw form, fp64, one wave per SIMD): a lane holds its knot's SYMMETRIC block -- the upper triangle,
// 45 values for X, 3E (3E + 1) / 2 for F -- where the other instantiations hold the knot's diagonal weights, loaded once per phase like
// them.  Q y is a lane-local mat-vec and d'Q d a lane-local quadratic form, both accumulated row by row with the columns in increasing
// index, in every lanes-per-problem mapping alike (only the segment sums differ between mappings, as without blocks); the chains start
// from the terms the diagonal code adds its product to, so a block that holds a diagonal alone (exact zeros beside it) gives the
// diagonal code's bits.  No step certificate (its Gershgorin rows assume a diagonal W) and no fp32 step decisions: every step is tested
// on the fp64 sums.  Every BQ line is under `if constexpr`: the other instantiations compile what they compiled without it.
// sym_index: where element (r, c) of a symmetric n x n block sits in its packed upper triangle (rows one after the other)
constexpr int sym_index(int n, int r, int c) { return r <= c ? r * n - r * (r - 1) / 2 + (c - r) : c * n - c * (c - 1) / 2 + (r - c); }

// KQ (costs that couple neighbouring knots -- force-rate and momentum-rate terms D'R D, D the first difference over knots: raw form,
// fp64, one wave per SIMD, diagonal per-knot weights): beside its knot's diagonal weights a lane holds the weights `off` between its
// knot t and knot t + 1, component by component (9 for X, 3E for F; exactly zero in the last knot's lane and in lanes without a knot)
// and those of the pair (t - 1, t), fetched from the previous lane once per phase.  (Q y)_t = diag_t y_t + off_{t-1} y_{t-1} + off_t y_{t+1}
// and d'Q d = sum_t diag_t d_t^2 + 2 off_t d_t d_{t+1} (lane t owns the pair): the neighbour lanes' y come by the wave shifts the motion
// step already uses for A_f -- in the force step they are its first exchange between knots -- and d_{t+1} likewise, once per trial of a
// step.  What a shift brings across the end of a segment is removed by keep_if, not
// by its zero weight: NaN x 0 is NaN, and a diverged problem's NaNs stay its own.  The coupling products are added behind the diagonal
// code's own term, so zero weights follow the diagonal kernel's path.  No step certificate (W + rho A_x'A_x is no longer block-diagonal
// per knot) and no fp32 step decisions.  Every KQ operation is under `if constexpr` (its few declarations beside them are dead in the
// other instantiations): those compile to the instructions they compiled to without it.
//
// CONE (the Euclidean projection onto the friction cone |f_xy| <= mu f_z, per-foot coefficients: both forms, fp64, one wave per SIMD,
// diagonal costs): the force step's projection is the nearest point of the cone instead of the reference's "SoC" step -- with
// s2 = fx^2 + fy^2: the origin for a step in the polar cone (fz <= 0, mu^2 s2 <= fz^2), the step itself inside the cone (fz >= 0,
// s2 <= mu^2 fz^2), otherwise t = (mu s + fz) / (mu^2 + 1) along the axis and mu t along f_xy.  The two tests are on squared
// quantities; the square root and the divisions are behind the wave-uniform ballot the reference's cone branch sits behind.  A lane
// loads its knot's coefficients mu[t][0 .. E) once per solve (ConeArgs; without an array every foot has SolverConsts::mu) and keeps
// them in registers.  No step certificate and no fp32 step decisions: every step is tested on the fp64 sums, as with BQ and KQ.  Every
// CONE operation is under `if constexpr`: the other instantiations compile what they compiled without it.
// (The cone KERNELS take their coefficients where the band kernels take their costs, as their one argument beside BatchArgs: a further
// argument of a kernel, even an empty struct, is one more temporary in it and reordered the block kernels' prologues.  That concerns
// the kernels' own parameter lists (biconvex_admm_inst.h).  admm_body itself takes the variant's struct as its single argument `ex`,
// whatever the shape: checked to leave every kernel's instructions what they were, tools/device_asm_diff.py.)
//
// FRAME (CONE about per-contact surface normals, ConeFrameArgs): the cone's axis is the unit normal n of the foot's contact at the lane's
// knot, world frame, instead of world z.  With fn = n.f, ft = f - fn n, s2 = |ft|^2 the three branches are CONE's with fn for fz --
// origin, the step's own bits, or k ft + t n with t = (mu s + fn) / (mu^2 + 1), k = mu t / s -- behind the same ballot.  The
// accumulation orders (fn = fma(nx, fx, fma(ny, fy, nz fz)), ft = fma(-fn, n, f), s2 = fma(ftx, ftx, fma(ftz, ftz, fty fty)), each
// output fma(t, n_i, k ft_i)) make every extra term an exact zero for n = (0, 0, 1): the cone kernel's values, up to the sign of a zero.
// A lane loads its knot's 3E normal components once per solve, beside the coefficients, and keeps them (the compiler rests them in
// accumulation registers; lanes without a force knot: world z).  The kernel does not normalise.  Every FRAME operation is under
// `if constexpr`, and its arguments come as the cone's do, in `ex`.
//
// AdmmCfg names one variant of the body: what admm_body is instantiated with.  SHAPE (CostShape, biconvex_kernels.h) says which Q and
// which projection -- one value, so a variant cannot be two shapes at once -- and with it which argument struct the variant's arrays
// come in (Extra; kDiag: an empty one).  What a shape's kernels are built for is asserted here from the shape's row of kShapes, the
// table the launches, plan_launch and the C-ABI read as well.
template <typename R_, int LPP_, int E_, bool RAW_, bool HASQF_, bool STEAL_ = false, bool XLDS_ = false, int WAVES_ = 1, CostShape SHAPE_ = kDiag, bool CLDS_ = false, bool MATES_ = false>
struct AdmmCfg {
    using R = R_;
    using Extra = ShapeExtra<SHAPE_>;
    static constexpr int LPP = LPP_, E = E_, WAVES = WAVES_;
    static constexpr bool RAW = RAW_, HASQF = HASQF_, STEAL = STEAL_, XLDS = XLDS_, FP64 = sizeof(R) == sizeof(double);
    static constexpr bool BQ = SHAPE_ == kBlocks, KQ = SHAPE_ == kBand, FRAME = SHAPE_ == kConeFrame, CONE = SHAPE_ == kCone || FRAME;
    static constexpr bool MW = WAVES > 1;
    static constexpr bool PARK = XLDS && !MW;      // (the LDS header is written by lane 0 and read by the whole problem: across waves that would take barriers)
    static constexpr bool CAN_CERT = FP64 && kShapes[SHAPE_].certifies;      // (see `certify` in the body)
    static constexpr bool BAND = !MW && !STEAL && XLDS && !RAW && LPP == 32 && E == 4 && FP64;      // (the headline kernel: see "fp32 step decisions" in the body)
    static constexpr bool CLDS = CLDS_;      // (the headline kernel with its certified loops' constants in LDS: see CLDS in the body)
    static_assert(!CLDS || BAND, "loop constants in LDS: a build of the headline kernel");
    static constexpr bool MATES = MATES_;    // (its waves in workgroups of eight, SIMD-mates keeping level: see MATES in the body)
    static_assert(!MATES || CLDS, "SIMD-mate workgroups: a geometry of the loop-constants build");
    static_assert(!kShapes[SHAPE_].fp64_only || FP64, "this cost shape: fp64 only");
    static_assert(!kShapes[SHAPE_].raw_only || RAW, "this cost shape: raw form only");
    static_assert(LPP * WAVES <= kShapes[SHAPE_].max_knots, "this cost shape: more lanes per problem than it has kernels for");
    static_assert(SHAPE_ == kDiag || (!STEAL && !XLDS && WAVES == 1), "cost shapes beside the diagonal: one wave per problem, one wave per SIMD");
    static_assert(!MW || (LPP == 64 && !STEAL && FP64), "several waves per problem: fp64, one problem per workgroup");
};
template <typename C>
__device__ __forceinline__ void admm_body(const BatchArgs &a, const typename C::Extra &ex = {}) {
    using R = typename C::R;
    constexpr int LPP = C::LPP, E = C::E, WAVES = C::WAVES;
    [[maybe_unused]] constexpr bool RAW = C::RAW, HASQF = C::HASQF, STEAL = C::STEAL, XLDS = C::XLDS, BQ = C::BQ, KQ = C::KQ, CONE = C::CONE, FRAME = C::FRAME, MW = C::MW, PARK = C::PARK;
    [[maybe_unused]] const auto &bq = ex, &kq = ex;      // (the names the BQ and the KQ / CONE / FRAME code reads its arrays by)
    [[maybe_unused]] constexpr bool MATES = C::MATES;
    extern __shared__ double lds_all[];
    // MATES: the wave's number in its workgroup and the doubles of one wave's LDS area -- wave-uniform, scalar registers
    // (every MATES line under `if constexpr`: the other instantiations compile what they compiled without it)
    [[maybe_unused]] unsigned wg_wave = 0, wave_doubles = 0;
    if constexpr (MATES) {
        wg_wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        wave_doubles = (unsigned)(loop_constants_lds_bytes(C::E, a.H) / sizeof(double));
    }
    // the wave's LDS: the array itself (a reference that no lambda has to capture) or, MATES, the wave's area in it
    decltype(auto) lds_raw = wave_lds<MATES>(lds_all, MATES ? wg_wave * wave_doubles : 0u);
    auto wave_ix = [&]() -> long { if constexpr (MATES) return (long)blockIdx.x * 8 + (long)wg_wave; else return (long)blockIdx.x; };
#ifdef BMPC_SIMD_STAMPS
    if constexpr (C::CLDS) simd_stamp(a.simd_stamps, true);
#endif
    constexpr int NF = 3 * E;           // force variables per knot
    constexpr int NB = RAW ? 9 : 3;     // bounded components per knot
    const int lane = threadIdx.x & 63, wv = MW ? (int)(threadIdx.x >> 6) : 0;
    const int t = MW ? (int)threadIdx.x : lane % LPP;           // knot owned by this lane
    const int seg = MW ? 0 : lane / LPP;
    const int H = a.H;
    long prob = MW ? (long)blockIdx.x : wave_ix() * (64 / LPP) + seg;      // (STEAL: the segment's FIRST problem)
    // STEAL: the lane's place in its segment decides what it owns; whether the segment has a problem at all is the `alive` mask's business
    const bool pvalid = seg < 64 / LPP && (STEAL || prob < a.B);      // (LPP = 21: lane 63 belongs to no segment)
    const bool kvalid = pvalid && t <= H;  // owns knot t (X block t)
    const bool rvalid = pvalid && t < H;   // owns dynamics row-block t and force block t
    const bool l0 = pvalid && t == 0;      // also owns the x_init rows 9H..9H+8
    const long nx = 9L * (H + 1), nf = (long)NF * H;
    const mask_t rvalid_m = __ballot(rvalid), kvalid_m = __ballot(kvalid);

    const R m = (R)a.c.m, rho = (R)a.c.rho, mu = (R)a.c.mu, beta = (R)a.c.beta;
    const double tol = a.c.tol, exit_tol = a.c.exit_tol;   // exit tests are evaluated in fp64 whatever R is
    const int maxit = a.c.maxit;
    const R rho2 = R(2) * rho;

    // Iterates at phase boundaries (X, F, P of this segment's problem) live in LDS, each lane touching
    // only its own knot's blocks (lane 0 also the x_init rows of P): HBM sees the inputs once and the
    // results once.
    // Layout: kLdsZeros zeros, then per segment the x_init rows' multipliers (kSegLds elements; lane 0 works on them) and one record
    // per KNOT, [X 9 | P 9 | F NF | R 9] (KL = knot_lds(E) = 39 elements for four feet, 33 for two: an odd stride, no two lanes of a
    // segment share a bank; the header below -- 12 doubles and 6 ints of lane 0 -- stays kSegLds long whatever E is).  Every block
    // of a lane -- lane 0's x_init block included -- is ONE address (the record's, less kSegLds elements) plus a constant, which the
    // LDS instructions carry as their immediate offset: one address register per lane instead of one per block (with separate
    // arrays per block the two-waves build kept reloading five of them from scratch memory).  R: the affine image of the FISTA
    // loops' x_k (XLDS).
    constexpr int KL = knot_lds(E);
    static_assert(9 + 9 + NF + 9 == KL && KL % 2 == 1 && kSegLds + KL <= kLdsZeros && kSegLds >= 9 && 12 + 6 / 2 <= kSegLds, "one LDS record per knot");
    R *zeros = reinterpret_cast<R *>(lds_raw);      // what a lane without a knot reads for x_k (XLDS)
    R *Sg = zeros + kLdsZeros + (long)seg * (kSegLds + (long)(H + 1) * KL) + (long)t * KL;
    R *PIg = Sg, *Xg = Sg + kSegLds, *Pg = Xg + 9, *Fg = Xg + 18, *Rg = Xg + 18 + NF;      // (PIg: lane 0's only)
    const R *Szr = rvalid ? Sg : zeros, *Szk = kvalid ? Sg : zeros;
    const R *Fz = Szr + kSegLds + 18, *RFz = Szr + kSegLds + 18 + NF, *Xz = Szk + kSegLds, *RXz = Szk + kSegLds + 18 + NF;
    // knot t <-> t +- 1 and the sums over a problem's knots: within the wave by DPP, across a workgroup's waves (MW) through LDS
    double *const xch = reinterpret_cast<double *>(zeros) + kLdsZeros + kSegLds + (long)(H + 1) * KL;      // MW: [2][WAVES][9] next, [2][WAVES][9] previous, [2][WAVES][2] sums
    int par_n = 0, par_p = 0, par_s = 0;
    auto shift_next = [&](const auto &v, auto &o) {      // o = v of knot t + 1 (0 behind the last lane)
        constexpr int N = (int)(sizeof(v) / sizeof(v[0]));
        UNROLL for (int l = 0; l < N; ++l) o[l] = from_next(v[l]);
        if (MW) {
            double *buf = xch + par_n * (WAVES * 9);
            if (lane == 0) { UNROLL for (int l = 0; l < N; ++l) buf[wv * 9 + l] = (double)v[l]; }
            __syncthreads();
            if (lane == 63 && wv + 1 < WAVES) { UNROLL for (int l = 0; l < N; ++l) o[l] = (R)buf[(wv + 1) * 9 + l]; }
            par_n ^= 1;
        }
    };
    auto shift_prev = [&](const auto &v, auto &o) {      // o = v of knot t - 1 (0 in front of the first lane)
        constexpr int N = (int)(sizeof(v) / sizeof(v[0]));
        UNROLL for (int l = 0; l < N; ++l) o[l] = from_prev(v[l]);
        if (MW) {
            double *buf = xch + 2 * WAVES * 9 + par_p * (WAVES * 9);
            if (lane == 63) { UNROLL for (int l = 0; l < N; ++l) buf[wv * 9 + l] = (double)v[l]; }
            __syncthreads();
            if (lane == 0 && wv > 0) { UNROLL for (int l = 0; l < N; ++l) o[l] = (R)buf[(wv - 1) * 9 + l]; }
            par_p ^= 1;
        }
    };
    auto sum2 = [&](double &s0, double &s1) {      // both sums over the problem's knots (seg_sum2's contract; MW: in every lane)
        seg_sum2<LPP>(s0, s1);
        if (MW) {
            double *buf = xch + 4 * WAVES * 9 + par_s * (WAVES * 2);
            if (lane == 0) { buf[2 * wv] = s0; buf[2 * wv + 1] = s1; }
            __syncthreads();
            double t0 = buf[0], t1 = buf[1];
            UNROLL for (int w = 1; w < WAVES; ++w) { t0 += buf[2 * w]; t1 += buf[2 * w + 1]; }
            s0 = t0; s1 = t1;
            par_s ^= 1;
        }
    };
    auto sum1 = [&](double &s0) {      // one of them, with sum2's bits for it
        seg_sum1<LPP>(s0);
        if (MW) {
            double *buf = xch + 4 * WAVES * 9 + par_s * (WAVES * 2);
            if (lane == 0) buf[2 * wv] = s0;
            __syncthreads();
            double t0 = buf[0];
            UNROLL for (int w = 1; w < WAVES; ++w) t0 += buf[2 * w];
            s0 = t0;
            par_s ^= 1;
        }
    };
    // The step certificate of a force phase: every lane of every live problem found its scaled Gershgorin row test
    // (`ok`) true -- then no step of the phase's FISTA loop can fail the backtracking test, and the loop runs without it.  Wave-
    // (MW: workgroup-) uniform.
    constexpr bool CAN_CERT = C::CAN_CERT;      // fp64 and a shape whose row of kShapes says so (BQ, KQ: the rows below assume a diagonal W; CONE: every step tested; fp32: the image noise does make the test fire, see the force step)
    auto certify = [&](bool ok, mask_t live) -> bool {
        if (!CAN_CERT || !a.certified_steps) return false;
        if (!MW) return (__ballot(!ok) & live) == 0;
        double f = ok ? 0.0 : 1.0;
        sum1(f);
        return __ballot(f != 0.0) == 0;
    };
    // ... and below which |d|^2 a certified loop hands the step to the tested one: the images A y + bPk are carried through the
    // momentum step, so rn - ry = A d + noise of a few ulp of the images; the certificate's margin absorbs the noise only while |d| is
    // not far below it.  s2: the lane's |bPk|^2 + (T / rho)|x_0|^2 (T / rho bounds |||A|||^2); the floor is the largest over the wave's
    // live problems (a scalar).
    auto cert_floor = [&](double s2, double Lh, mask_t live) {
        sum1(s2);
        const double f = lanes(live) ? s2 * kCertFloor * ((double)rho / Lh) : 0.0;
        constexpr int NS = LPP == 21 ? 3 : 64 / LPP;
        double m = 0.0;
        UNROLL for (int k = 0; k < NS; ++k) m = fmax(m, lane_bcast(f, LPP == 21 ? 16 * (k + 1) : k * LPP));
        return m;
    };
    // fp32 step decisions: a FISTA step takes retry (cv > (L/2) g2), exit (g2 < tol^2) and, in the certified
    // force loop, the floor test (g2 < floor2) from fp32 segment sums (seg_sum2_f32: 12 instead of 30 instructions at 32 lanes) when
    // for every live problem of the wave both comparisons are clear of their thresholds by kBand relative and the g2 sum lies in
    // [1e-24, 1e30]; the fp32 sums are within 5e-7 of the exact ones there, so each such decision is the one the fp64 sums make.
    // Otherwise the wave runs the fp64 sums and the reference expression, as it did without the shortcut.  The bound holds for sums of
    // non-negative terms: a phase takes the shortcut only with rho >= 0 and no negative weight in the wave (`banded`), and never under
    // bmpc_set_exact_step_decisions(1).  One instantiation takes it: the two-waves-per-SIMD build of the 32-lane, four-feet kernel in
    // the harness form -- the benchmark's kernel, the one whose gain (3.37 -> 3.30 ms), unchanged iterates and unchanged registers and
    // scratch (40 bytes per lane, none inside the loops) were checked.  In the other single-wave builds the same
    // source moved the compiler's register allocation (scratch of the 16- / 21-lane and two-feet kernels 40 -> 116, 32 -> 100, 8 -> 76
    // bytes per lane, reloads inside the FISTA loops), the rounding of the iterates (two feet, 21 lanes) or the time (the work-stealing
    // kernel, 27.6 -> 29.6 ms): they keep the fp64 sums, as do the workgroup kernels (MW) and the fp32 kernel.
    constexpr bool BAND = C::BAND;
    [[maybe_unused]] constexpr bool CLDS = C::CLDS;
    constexpr double kBand = 1e-5;
    // (1 - kBand) x and (1 + kBand) x as floats, wave-uniform (scalar registers): thresholds that need no range check, g2 is confined
    auto band_u = [](double x, float &lo, float &hi) {
        lo = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint((float)(x * (1.0 - kBand)))));
        hi = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint((float)(x * (1.0 + kBand)))));
    };
    // ... of a step constant L/2, per lane: NaN (no comparison clear) outside [1e-3, 1e30], where the products could leave fp32's range
    auto band_L = [](double Lh, float &lo, float &hi) {
        const bool in = Lh >= 1e-3 && Lh <= 1e30;
        lo = in ? (float)(Lh * (1.0 - kBand)) : __builtin_nanf("");
        hi = in ? (float)(Lh * (1.0 + kBand)) : __builtin_nanf("");
    };
    float t2lo = 0.0f, t2hi = 0.0f;
    if constexpr (BAND) band_u(tol * tol, t2lo, t2hi);
    // Global arrays are addressed as a WAVE-UNIFORM base (the block of the wave's first problem: scalar registers) plus a 32-bit
    // per-lane byte offset (problem within the wave, knot): `global_load v, v_off, s[base]`.  A 64-bit pointer per lane and array
    // -- what `a.X + pb * nx + 9 * t` makes -- held some thirty vector registers over both FISTA loops, and they were what the
    // fp32 build (256 registers, two waves per SIMD) parked in scratch memory.  Every lane's offset is that of an EXISTING
    // element (lanes past the horizon take the last knot's, lanes of a padding problem the wave's first problem): the loads
    // are unconditional -- straight-line code in which base + offset folds into the instruction, instead of some sixty
    // exec-masked blocks each needing the address as a 64-bit register pair -- and what a lane has no business with is
    // replaced by zero after the load (ldz).  Stores stay conditional.
    // (MATES: a wave of the last workgroup whose problems all lie beyond B -- one-wave workgroups have no such wave -- runs the prologue's
    // unconditional loads on the batch's first problems; no lane of it is pvalid, so it stores nothing and leaves the ADMM loop at once)
    const long wave0 = STEAL ? 0L : (MW ? (long)blockIdx.x : [&]() -> long {
        if constexpr (MATES) { const long w = wave_ix() * (64 / LPP); return w < a.B ? w : 0L; } else return wave_ix() * (64 / LPP); }());
    unsigned sl = STEAL ? (unsigned)(pvalid && prob < a.B ? prob : 0) : (pvalid ? (unsigned)seg : 0u);      // STEAL: the problem index itself
    const unsigned tk = (unsigned)(t <= H ? t : H), tr = (unsigned)(t < H ? t : H - 1);
    struct Off { unsigned X, PI, F, K, P9; };
    auto make_off = [&](unsigned slv) {
        Off o;
        o.X = 8u * (slv * (unsigned)nx + 9u * tk);                  // X, P, Qx, qx, lbx, ubx: [B][9 (H + 1)]
        o.PI = 8u * (slv * (unsigned)nx + 9u * (unsigned)H);
        o.F = 8u * (slv * (unsigned)nf + (unsigned)NF * tr);        // F, Qf, qf: [B][3 E H]
        o.K = 8u * (slv * (unsigned)H + tr);                        // dt: [B][H]; cnt_plan: E * 4 doubles per entry
        o.P9 = 8u * 9u * slv;                                        // x_init, X_ter: [B][9]
        return o;
    };
    unsigned oX, oPI, oF, oK, oP9;
    auto set_offsets = [&]() { const Off o = make_off(sl); oX = o.X; oPI = o.PI; oF = o.F; oK = o.K; oP9 = o.P9; };
    set_offsets();
    double *const Xu = a.X + wave0 * nx, *const Fu = a.F + wave0 * nf, *const Pu = a.P + wave0 * nx;
    const double *const xinit_u = a.x_init + wave0 * 9;

    if (lane < kLdsZeros) zeros[lane] = R(0);
    // MATES: the mailbox behind the eight waves' areas; every wave of the workgroup -- one whose problems lie beyond B too -- publishes its
    // SIMD in front of the barrier, meets the barrier, and then looks for the one other wave with the same number
    [[maybe_unused]] unsigned my_simd = 0;
    if constexpr (MATES) {
        int *const mailbox = reinterpret_cast<int *>(lds_all + 8u * wave_doubles);
        my_simd = (unsigned)__builtin_amdgcn_s_getreg(4 | 4 << 6 | 1 << 11);      // HW_REG_HW_ID bits 5:4
        if (lane == 0) { mailbox[wg_wave] = (int)my_simd; mailbox[8 + wg_wave] = 0; }
    }
    __syncthreads();
    [[maybe_unused]] int mate = -1;      // the mate's number in the workgroup (wave-uniform); -1: none, or the rule is off
    if constexpr (MATES) {
        if ((a.force_foot_pairs & 2) != 0) {
            const int *const mailbox = reinterpret_cast<const int *>(lds_all + 8u * wave_doubles);
            int found = 0;
            UNROLL for (int w = 0; w < 8; ++w) {
                const unsigned id = (unsigned)__builtin_amdgcn_readfirstlane(mailbox[w]);
                if ((unsigned)w != wg_wave && id == my_simd) { mate = w; ++found; }
            }
            if (found != 1) mate = -1;
        }
    }
    // ... and at the head of a phase, the n-th of the solve counted from 1 (kMateDone: behind the last): one word written, one read, one
    // s_setprio -- see MATES above
    [[maybe_unused]] auto mate_boundary = [&](int n) {
        if constexpr (MATES) {
            if (mate >= 0) {
                int *const box = reinterpret_cast<int *>(lds_all + 8u * wave_doubles) + 8;
                __hip_atomic_store(box + wg_wave, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);      // (every lane the same word: no exec mask to make)
                const int m = __builtin_amdgcn_readfirstlane(__hip_atomic_load(box + mate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                if (m >= n && m != kMateDone) __builtin_amdgcn_s_setprio(1);
                else __builtin_amdgcn_s_setprio(0);
            }
        }
    };
    const double *const cmtab = a.cmtab;      // (wave-uniform reads.  The loop-constants build takes them through the scalar cache, uniform_load; as plain
                                              // loads, everywhere else, hipcc makes them per-lane global loads of one address)

    R dt = ldz<R>(a.dt + wave0 * H, oK, 0, rvalid);
    R dtp;  // dt of knot t-1 (0 for t == 0: previous lane is a dead/terminal lane)
    { const R d1[1] = {dt}; R o1[1]; shift_prev(d1, o1); dtp = o1[0]; }
    const bool cold = a.cold_start != 0;      // 1: fresh solver object (iterates and step constants reset); 2: iterates only --
    const bool fresh_L = a.cold_start == 1;   // FISTA's L_ is set in the constructor and survives every optimize call (fista.hpp:52)
    const double L0x = a.L0_x, L0f = a.L0_f;      // (locals: read through `a` inside the lambda below, the two arguments got a stack copy)
    R L_x, L_f;
    int n_admm = 0, it_f = 0, it_x = 0, bt_f = 0, bt_x = 0, status = 0;
    double last_viol = 0.0;
    // XLDS: the bookkeeping of a problem -- step constants, counters, the last violation: segment-uniform values every lane carries --
    // is in registers only during the phase that changes it; across the OTHER phase's FISTA loop it rests in the problem's LDS
    // header (behind the x_init block; lane 0 writes, every lane of the segment reads the same words back).  In registers throughout
    // they were what the 256-register build stored to scratch memory in every ADMM iteration.
    static_assert(!XLDS || sizeof(R) == sizeof(double), "the LDS header holds doubles");
    // (the header's address is made where it is used, from the lane number as a value the optimiser cannot trace: hoisted out of
    // the ADMM loop it was itself kept in scratch memory)
    auto header = [&]() {
        const int sg = (int)(opaque_copy((unsigned)lane) / (unsigned)LPP);
        return reinterpret_cast<double *>(zeros) + kLdsZeros + (long)(sg < 64 / LPP ? sg : 0) * (kSegLds + (long)(H + 1) * KL);
    };
    auto lds_fence = [&]() { asm volatile("" ::: "memory"); };       // (the compiler may not carry a parked value past this in a register)
    // (CLDS: lane 0's stores too take the address from header(), not from Sg, which is a value of the whole kernel that hipcc reloads from
    // scratch memory in front of every use -- see "phase prologues" below)
    auto park_x = [&]() {      // before the force loop: everything the motion step and the end of the ADMM iteration work on
        if (l0) { double *Hd; if constexpr (C::CLDS) Hd = header(); else Hd = reinterpret_cast<double *>(Sg);      // (lane 0's record starts at the header)
                  int *Hi = reinterpret_cast<int *>(Hd + 12);
                  Hd[9] = (double)L_x; Hd[11] = last_viol; Hi[0] = it_x; Hi[1] = bt_x; Hi[2] = n_admm; Hi[3] = status; }
        lds_fence();
    };
    auto park_f = [&]() {      // before the motion step: what the force loop works on
        if (l0) { double *Hd; if constexpr (C::CLDS) Hd = header(); else Hd = reinterpret_cast<double *>(Sg);
                  int *Hi = reinterpret_cast<int *>(Hd + 12); Hd[10] = (double)L_f; Hi[4] = it_f; Hi[5] = bt_f; }
        lds_fence();
    };
    auto load_xloop = [&]() {      // in front of the motion loop
        lds_fence();
        const double *Hd = header(); const int *Hi = reinterpret_cast<const int *>(Hd + 12);
        L_x = (R)Hd[9]; it_x = Hi[0]; bt_x = Hi[1];
    };
    auto load_rest = [&]() {       // behind it: the end of the ADMM iteration reads and updates all of it
        lds_fence();
        const double *Hd = header(); const int *Hi = reinterpret_cast<const int *>(Hd + 12);
        last_viol = Hd[11]; n_admm = Hi[2]; status = Hi[3]; L_f = (R)Hd[10]; it_f = Hi[4]; bt_f = Hi[5];
    };
    // CLDS (the loop-constants build, see the motion step): the lane number as the hardware counts it, counted where it is needed -- on an
    // opaque zero, or it is counted once per kernel -- and from it, in the phase that uses them, the address of the constants of the lane's
    // knot (as a byte offset into LDS; lanes outside `own` read the zeros) and of its record.  Made from `lane` they are values of the
    // whole kernel, which hipcc parks in scratch memory and reads back inside the loops.
    [[maybe_unused]] auto lane_id = [&]() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, opaque_zero())); };
    // A lane outside `own` reads its zeros where the record of the knot it would own -- the stride going on past the horizon -- falls in
    // the LDS banks: element (that record's element index) mod 32 of the zeros at the front of LDS.  The lanes of a 32-lane segment then
    // sit on 32 different bank pairs in every read of the constants, and those of each group of 16 on 16 (19 is odd; DESIGN.md section
    // 4 and tools/lds_bank_model.py).  At one address for all of them -- element 0 -- they met a knot lane's bank in most of these
    // reads.  The last element read is 31 + 18 < kLdsZeros.
    static_assert(!CLDS || (kLoopConstLds % 2 == 1 && 31 + kLoopConstLds <= kLdsZeros), "idle lanes read exact zeros, on banks of their own");
    [[maybe_unused]] auto consts_offset = [&](mask_t own) {
        const unsigned ln = opaque_copy(lane_id());
        const unsigned e = (unsigned)(kLdsZeros + 2 * (kSegLds + (H + 1) * KL)) + (ln / (unsigned)LPP * (unsigned)(H + 1) + ln % (unsigned)LPP) * (unsigned)kLoopConstLds;
        return 8u * (lanes(own) ? e : e & 31u);
    };
    [[maybe_unused]] auto knot_record = [&]() {      // (Xg, made again where a store needs it, as header() is: held across a loop it is one register too many)
        const unsigned ln = opaque_copy(lane_id());
        return reinterpret_cast<R *>(lds_raw) + kLdsZeros + (long)(ln / (unsigned)LPP) * (kSegLds + (long)(H + 1) * KL) + (long)(ln % (unsigned)LPP) * KL + kSegLds;
    };
    // CLDS, phase prologues (everything of the ADMM iteration outside the FISTA loops: DESIGN.md section 4, "Phase prologues").  The blocks of
    // the lane's record are read there UNCONDITIONALLY, as one batch per block behind one wait (lds_block, biconvex_lanes.h), from one
    // address per region of the code, made in that region: record_or_front.  Written as `kvalid ? Xg[l] : 0` every element was an
    // exec-masked block of its own that first reloaded the record's address from scratch memory and waited for it (about 140 dependent
    // round trips per ADMM iteration).  A lane in `own` gets its record (its X block; P, F, R behind it as in Xg); a lane outside reads
    // at the front of LDS, where consts_offset sends its idle lanes: element (its record's element index) mod 32, so the lanes of a
    // segment stay on 32 different bank pairs.  What it finds there -- zeros, then the first problem's header: at most element
    // 31 + 18 + NF < kLdsZeros + kSegLds -- is never used: every block read this way goes through a select on the lane's own predicate.
    static_assert(!CLDS || 31 + 18 + NF <= kLdsZeros + kSegLds, "lanes without a knot read inside the wave's LDS");
    [[maybe_unused]] auto record_or_front = [&](mask_t own) {
        const unsigned ln = opaque_copy(lane_id());
        const unsigned e = (unsigned)(kLdsZeros + kSegLds) + ln / (unsigned)LPP * (unsigned)(kSegLds + (H + 1) * KL) + ln % (unsigned)LPP * (unsigned)KL;
        return reinterpret_cast<R *>(reinterpret_cast<char *>(lds_raw) + 8u * (lanes(own) ? e : e & 31u));
    };
    // the problem `sl` names (every offset set) comes on chip: step constants, iterates, counters (lanes of the segments in m)
    auto load_problem = [&](mask_t m) {
        const bool on = lanes(m);
        const R nLx = (R)(fresh_L ? L0x : *at(a.L_x + wave0, 8u * sl)), nLf = (R)(fresh_L ? L0f : *at(a.L_f + wave0, 8u * sl));
        if (on) { L_x = nLx; L_f = nLf; n_admm = 0; it_f = 0; it_x = 0; bt_f = 0; bt_x = 0; status = 0; last_viol = 0.0; }
        if (cold) {  // KinoDynMP::set_warm_starts (kino_dyn.cpp:83-99): X = tile(x_init), F = 0, P = 0
            if (on && kvalid) { UNROLL for (int l = 0; l < 9; ++l) Xg[l] = (R)at(xinit_u, oP9)[l]; }
            if (on && rvalid) {
                UNROLL for (int j = 0; j < NF; ++j) Fg[j] = R(0);
                UNROLL for (int l = 0; l < 9; ++l) Pg[l] = R(0);
            }
            if (on && l0) { UNROLL for (int l = 0; l < 9; ++l) PIg[l] = R(0); }
        } else {     // set_warm_start_vars: bring the caller's iterates on chip
            if (on && kvalid) { UNROLL for (int l = 0; l < 9; ++l) Xg[l] = (R)at(Xu, oX)[l]; }
            if (on && rvalid) {
                UNROLL for (int j = 0; j < NF; ++j) Fg[j] = (R)at(Fu, oF)[j];
                UNROLL for (int l = 0; l < 9; ++l) Pg[l] = (R)at(Pu, oX)[l];
            }
            if (on && l0) { UNROLL for (int l = 0; l < 9; ++l) PIg[l] = (R)at(Pu, oPI)[l]; }
        }
    };
    // ... and its results leave: one pass from LDS to the output blocks
    auto store_problem = [&](mask_t m) {
        const bool on = lanes(m);
        if (on && kvalid) { UNROLL for (int l = 0; l < 9; ++l) at(Xu, oX)[l] = (double)Xg[l]; }
        if (on && rvalid) {
            UNROLL for (int j = 0; j < NF; ++j) at(Fu, oF)[j] = (double)Fg[j];
            UNROLL for (int l = 0; l < 9; ++l) at(Pu, oX)[l] = (double)Pg[l];
        }
        if (on && l0) { UNROLL for (int l = 0; l < 9; ++l) at(Pu, oPI)[l] = (double)PIg[l]; }
        if (on && l0) {
            *at(a.L_x + wave0, 8u * sl) = (double)L_x;
            *at(a.L_f + wave0, 8u * sl) = (double)L_f;
            if (a.dyn_viol) *at(a.dyn_viol + wave0, 8u * sl) = last_viol;
            if (a.stats) {
                int *s = a.stats + (wave0 + sl) * kStats;
                s[0] = n_admm; s[1] = it_f; s[2] = it_x; s[3] = bt_f; s[4] = bt_x; s[5] = status;
            }
        }
    };
    mask_t alive = __ballot(pvalid && prob < a.B);
    if (STEAL) {
        L_x = (R)L0x; L_f = (R)L0f;      // (lanes of no problem: finite step constants, whatever they then compute is masked)
        load_problem(alive);
    } else {
        // (the plain kernels keep the straight-line prologue and epilogue they were tuned with: written through the lambdas above --
        // the same operations under a lane mask -- the headline kernel came out 2.5 % slower, 4.09 against 3.98 ms on one box)
        L_x = (R)(fresh_L ? L0x : *at(a.L_x + wave0, 8u * sl));
        L_f = (R)(fresh_L ? L0f : *at(a.L_f + wave0, 8u * sl));
        if (cold) {  // KinoDynMP::set_warm_starts (kino_dyn.cpp:83-99): X = tile(x_init), F = 0, P = 0
            if (kvalid) { UNROLL for (int l = 0; l < 9; ++l) Xg[l] = (R)at(xinit_u, oP9)[l]; }
            if (rvalid) {
                UNROLL for (int j = 0; j < NF; ++j) Fg[j] = R(0);
                UNROLL for (int l = 0; l < 9; ++l) Pg[l] = R(0);
            }
            if (l0) { UNROLL for (int l = 0; l < 9; ++l) PIg[l] = R(0); }
        } else {     // set_warm_start_vars: bring the caller's iterates on chip
            if (kvalid) { UNROLL for (int l = 0; l < 9; ++l) Xg[l] = (R)at(Xu, oX)[l]; }
            if (rvalid) {
                UNROLL for (int j = 0; j < NF; ++j) Fg[j] = (R)at(Fu, oF)[j];
                UNROLL for (int l = 0; l < 9; ++l) Pg[l] = (R)at(Pu, oX)[l];
            }
            if (l0) { UNROLL for (int l = 0; l < 9; ++l) PIg[l] = (R)at(Pu, oPI)[l]; }
        }
    }

    // CONE: the friction coefficients of this lane's knot, one per foot, for the whole solve (lanes without a force knot: 1, their
    // forces are zero and stay zero)
    [[maybe_unused]] R muf[CONE ? E : 1];
    if constexpr (CONE) {
        const auto &cn = kq;      // (ConeArgs: see the signature)
        if (cn.mu) {
            const unsigned oM = 8u * (sl * (unsigned)cn.smu + (unsigned)E * tr);
            UNROLL for (int n = 0; n < E; ++n) { const double v = at(cn.mu + wave0 * cn.smu, oM)[n]; muf[n] = rvalid ? (R)v : R(1); }
        } else {
            UNROLL for (int n = 0; n < E; ++n) muf[n] = mu;
        }
    }
    // FRAME: ... and the unit normals of its contacts, three components per foot (lanes without a force knot read an existing element,
    // as above, and take world z)
    [[maybe_unused]] R nrm[FRAME ? NF : 1];
    if constexpr (FRAME) {
        const unsigned oN = 8u * (sl * (unsigned)kq.snormals + (unsigned)NF * tr);
        UNROLL for (int j = 0; j < NF; ++j) { const double v = at(kq.normals + wave0 * kq.snormals, oN)[j]; nrm[j] = rvalid ? (R)v : R(j % 3 == 2 ? 1 : 0); }
    }

    // BAND: how many force and motion phases of the problem ran the certified loop from their first iteration (BatchArgs::cert_phases),
    // counted by lane 0 in two ints of LDS nothing else uses -- the F block of knot H's record (the last knot has no forces) -- once per
    // phase, in front of its FISTA loop; written out once, behind the last ADMM iteration.
    [[maybe_unused]] int *const certn = reinterpret_cast<int *>(Sg + kSegLds + (long)H * KL + 18);      // (lane 0's: its record is the segment's first)
    if constexpr (BAND) { if (l0) { certn[0] = 0; certn[1] = 0; } }
    [[maybe_unused]] auto cert_count = [&]() -> int * {      // certn where a phase counts (CLDS: from header(), see "phase prologues")
        if constexpr (CLDS) return reinterpret_cast<int *>(header() + kSegLds + (long)H * KL + 18);
        else return certn;
    };
    // CLDS: the unit map of the force loop's two feet per lane (see the force step), made ONCE per solve: it follows from the contact plan
    // and H alone -- a foot is in contact where an = c (dt / m) is not zero -- and neither changes within a solve.  A scatter through 64
    // bytes of LDS per segment, the F block of knot H's record behind the two ints of cert_count (the last knot has no forces: every
    // store to an F block is a force knot's or a unit's, t < H, so nothing but this writes there until the kernel ends); an entry: knot |
    // rank << 5 | contact feet << 8, 0x8000 = no unit.  Behind its 32 entries the segment's mask of knots with two units, which an
    // unsettled iteration reads.  `pair_fits` (wave-uniform): at most 32 units in each of the wave's problems.
    // (The address from the lane number counted in place, as knot_record's: header() reads `lane`, which hipcc reloads from scratch memory.)
    [[maybe_unused]] auto unit_map = [&]() {
        const unsigned ln = opaque_copy(lane_id());
        return reinterpret_cast<unsigned short *>(reinterpret_cast<double *>(lds_raw) + kLdsZeros + (long)(ln / (unsigned)LPP) * (kSegLds + (long)(H + 1) * KL) + kSegLds + (long)H * KL + 18 + 1);
    };
    [[maybe_unused]] bool pair_fits = false;
    if constexpr (CLDS) {
        if ((MATES ? (a.force_foot_pairs & 1) : a.force_foot_pairs) != 0) {      // (MATES: bit 1 is the rule's switch)
            const double *const cnt0 = a.cnt_plan + wave0 * H * (E * 4);
            unsigned cmk = 0;      // the knot's contact feet, one bit per foot
            UNROLL for (int n = 0; n < E; ++n) cmk |= ldz<R>(cnt0, oK * (unsigned)(E * 4), 4 * n, rvalid) * (dt / m) == R(0) ? 0u : 1u << n;
            const bool two = __popc(cmk) > 2;
            const mask_t two_m = __ballot(two);
            pair_fits = H + __popc((unsigned)two_m) <= 32 && H + __popc((unsigned)(two_m >> 32)) <= 32;
            const unsigned ln = opaque_copy(lane_id()), tl = ln & 31u;
            const unsigned tw = ln < 32u ? (unsigned)two_m : (unsigned)(two_m >> 32);
            const unsigned start = tl + (unsigned)__popc(tw & ((1u << tl) - 1u));      // (<= 31 for every knot lane where the map is used: pair_fits)
            unsigned short *mp = unit_map();
            mp[tl] = (unsigned short)0x8000u;
            if (tl == 0u) reinterpret_cast<unsigned *>(mp)[16] = tw;
            lds_fence();
            if (pair_fits && rvalid) {
                mp[start] = (unsigned short)(tl | cmk << 8);
                if (two) mp[start + 1u] = (unsigned short)(tl | 32u | cmk << 8);
            }
            lds_fence();
        }
    }

    for (int it = 0; STEAL || it < a.c.num_iters; ++it) {
        if (alive == 0) break;
        // contact data of this knot: flags c_n, positions r_n  (centroidal.cpp:39-49); re-read in
        // each phase (L2-resident) rather than held in registers across the FISTA loops
        const double *const cnt_u = a.cnt_plan + wave0 * H * (E * 4);

        // =================================================================== F step
        {
            if constexpr (MATES) mate_boundary(2 * it + 1);
            if (PARK) park_x();
            const unsigned ph = opaque_zero();      // see opaque_zero (biconvex_lanes.h): the inputs are re-read in each phase
            // XLDS: ... and their offsets re-made from the problem's index (hoisted out of the ADMM loop they were a dozen registers
            // that the 256-register build kept in scratch memory)
            const unsigned sl_ = XLDS ? opaque_copy(sl) : sl;
            const Off o = XLDS ? make_off(sl_) : Off{oX, oPI, oF, oK, oP9};
            const unsigned oC = o.K * (unsigned)(E * 4);
            R c[E], r[E][3];
            UNROLL for (int n = 0; n < E; ++n) {
                c[n] = ldz<R>(cnt_u, oC + ph, 4 * n, rvalid);
                UNROLL for (int k = 0; k < 3; ++k) r[n][k] = ldz<R>(cnt_u, oC + ph, 4 * n + 1 + k, rvalid);
            }
            R X[9];
            [[maybe_unused]] R *rec = nullptr;      // CLDS: the lane's record, or the front of LDS (see "phase prologues"): this prologue's one address
            [[maybe_unused]] R Pv[CLDS ? 6 : 1], F0[CLDS ? NF : 1];
            if constexpr (CLDS) {
                rec = record_or_front(kvalid_m);
                lds_block(rec, X, kvalid);
                lds_batch(rec + 9 + 3, Pv);      // (selected with the sum it enters, below)
                lds_block(rec + 18, F0, rvalid);
            } else {
            UNROLL for (int l = 0; l < 9; ++l) X[l] = kvalid ? Xg[l] : R(0);
            }
            // bPk rows 9t+3..8 = -b_x + P, b_x = X_{t+1} - X_t (+g dt)   (centroidal.cpp:60-65)
            R bpk[6], Xv[6], Xvn[6];
            UNROLL for (int k = 0; k < 6; ++k) Xv[k] = X[3 + k];
            shift_next(Xv, Xvn);
            UNROLL for (int k = 0; k < 6; ++k) {
                const R xn = Xvn[k];
                R bx = xn - X[3 + k];
                if (k == 2) bx += R(kGravity) * dt;
                if constexpr (CLDS) bpk[k] = rvalid ? (-bx + Pv[k]) : R(0);
                else bpk[k] = rvalid ? (-bx + Pg[3 + k]) : R(0);
            }
            // A_x entries of this knot (centroidal.cpp:67-81)
            R an[E], sp[E][3];
            UNROLL for (int n = 0; n < E; ++n) {
                an[n] = c[n] * (dt / m);
                UNROLL for (int k = 0; k < 3; ++k) sp[n][k] = c[n] * (X[k] - r[n][k]) * dt;
            }
            // The gradient is carried as HALF of itself, gh = Q y + q/2 + rho A^T(A y + bPk), and the step as y - (2/L) gh:
            // scaling by two is exact in binary floating point, so every iterate has the bits of the reference's
            // y - g/L, and the doubled copies of the weights (2 Q, 2 rho) need no registers.
            R wf[NF], qf[HASQF ? NF : 1];
            constexpr int NW = BQ ? NF * (NF + 1) / 2 : 1;
            [[maybe_unused]] R Wb[NW];      // BQ: the knot's block, its upper triangle (sym_index)
            if constexpr (BQ) {
                UNROLL for (int j = 0; j < NF; ++j) {
                    wf[j] = R(0);      // (unused)
                    if (HASQF) qf[j] = R(0.5) * ldz<R>(a.qf + wave0 * nf, o.F + ph, j, rvalid);
                }
                if (bq.Qf_blk) {
                    const unsigned oB = 8u * (sl_ * (unsigned)bq.sQf_blk + (unsigned)(NF * NF) * tr) + ph;
                    UNROLL for (int r = 0; r < NF; ++r) {
                        UNROLL for (int cc = r; cc < NF; ++cc) Wb[sym_index(NF, r, cc)] = ldz<R>(bq.Qf_blk + wave0 * bq.sQf_blk, oB, r * NF + cc, rvalid);
                    }
                } else {      // this side has its diagonal only: the block with exact zeros beside it
                    UNROLL for (int k = 0; k < NW; ++k) Wb[k] = R(0);
                    UNROLL for (int j = 0; j < NF; ++j) Wb[sym_index(NF, j, j)] = ldz<R>(a.Qf + wave0 * nf, o.F + ph, j, rvalid);
                }
            } else {
            UNROLL for (int j = 0; j < NF; ++j) {
                wf[j] = RAW ? ldz<R>(a.Qf + wave0 * nf, o.F + ph, j, rvalid)
                            : ldz<R>(a.W_F + wave0 * a.sW_F, 8u * (sl_ * (unsigned)a.sW_F + (unsigned)NF * tr) + ph, j, rvalid);
                if (HASQF) qf[j] = R(0.5) * ldz<R>(a.qf + wave0 * nf, o.F + ph, j, rvalid);
            }
            }
            // KQ: the weights between knots t and t + 1 (of) and t - 1 and t (ofp); a lane's place decides which neighbours it has
            [[maybe_unused]] R of[KQ ? NF : 1], ofp[KQ ? NF : 1];
            [[maybe_unused]] const int fnm = pvalid && t + 1 < H ? -1 : 0, fpm = rvalid && t >= 1 ? -1 : 0;
            if constexpr (KQ) {
                if (kq.Qf_off) {
                    const unsigned oB = 8u * (sl_ * (unsigned)kq.sQf_off + (unsigned)NF * (unsigned)(t + 1 < H ? t : (H >= 2 ? H - 2 : 0))) + ph;
                    UNROLL for (int j = 0; j < NF; ++j) of[j] = ldz<R>(kq.Qf_off + wave0 * kq.sQf_off, oB, j, fnm != 0);
                } else {
                    UNROLL for (int j = 0; j < NF; ++j) of[j] = R(0);
                }
                shift_prev(of, ofp);
                UNROLL for (int j = 0; j < NF; ++j) ofp[j] = keep_if(ofp[j], fpm);
            }
            // the step certificate: M = W + rho A_x'A_x is block-diagonal per knot; with dg = diag(M), u = |A| dg, v = |A|' u the lane's
            // rows pass if W_j dg_j + rho v_j <= T dg_j (tools/certify_rate.py restates this)
            bool cert = false;
            double floor2 = 0.0;
            if (CAN_CERT && a.certified_steps) {
                const double Lh0 = (double)L_f * 0.5, T = Lh0 * (1.0 - kCertEta);
                double dg[NF], u[6] = {0, 0, 0, 0, 0, 0}, x2 = 0.0, b2 = 0.0;
                UNROLL for (int n = 0; n < E; ++n) {
                    const double a0 = fabs((double)an[n]), s0 = (double)sp[n][0], s1 = (double)sp[n][1], s2 = (double)sp[n][2];
                    const double q = a0 * a0 + s0 * s0 + s1 * s1 + s2 * s2;
                    dg[3 * n] = (double)wf[3 * n] + (double)rho * (q - s0 * s0);
                    dg[3 * n + 1] = (double)wf[3 * n + 1] + (double)rho * (q - s1 * s1);
                    dg[3 * n + 2] = (double)wf[3 * n + 2] + (double)rho * (q - s2 * s2);
                    UNROLL for (int k = 0; k < 3; ++k) u[k] += a0 * dg[3 * n + k];
                    u[3] += fabs(s2) * dg[3 * n + 1] + fabs(s1) * dg[3 * n + 2];
                    u[4] += fabs(s0) * dg[3 * n + 2] + fabs(s2) * dg[3 * n];
                    u[5] += fabs(s1) * dg[3 * n] + fabs(s0) * dg[3 * n + 1];
                }
                bool ok = true;
                UNROLL for (int n = 0; n < E; ++n) {
                    const double a0 = fabs((double)an[n]), s0 = fabs((double)sp[n][0]), s1 = fabs((double)sp[n][1]), s2 = fabs((double)sp[n][2]);
                    const double v[3] = {a0 * u[0] + s2 * u[4] + s1 * u[5], a0 * u[1] + s2 * u[3] + s0 * u[5], a0 * u[2] + s1 * u[3] + s0 * u[4]};
                    UNROLL for (int k = 0; k < 3; ++k) ok = ok && (double)wf[3 * n + k] * dg[3 * n + k] + (double)rho * v[k] <= T * dg[3 * n + k];
                }
                if constexpr (CLDS) { UNROLL for (int j = 0; j < NF; ++j) x2 += (double)F0[j] * (double)F0[j]; }      // (a lane without forces: exact zeros, x2 stays +0.0)
                else
                if (rvalid) { UNROLL for (int j = 0; j < NF; ++j) x2 += (double)Fg[j] * (double)Fg[j]; }      // (x_0: the F block)
                UNROLL for (int k = 0; k < 6; ++k) b2 += (double)bpk[k] * (double)bpk[k];
                cert = certify(ok, alive);
                if (cert) floor2 = cert_floor(b2 + (T / (double)rho) * x2, Lh0, alive);
            }
            if constexpr (BAND) { if (cert && l0 && lanes(alive)) ++cert_count()[0]; }
            // u = A v + bPk on rows 9t+3..8
            auto applyA = [&](const R (&v)[NF], R (&u)[6]) {
                R s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0;
                UNROLL for (int n = 0; n < E; ++n) {
                    const R vx = v[3 * n], vy = v[3 * n + 1], vz = v[3 * n + 2];
                    s0 += an[n] * vx; s1 += an[n] * vy; s2 += an[n] * vz;
                    s3 += sp[n][2] * vy - sp[n][1] * vz;
                    s4 += sp[n][0] * vz - sp[n][2] * vx;
                    s5 += sp[n][1] * vx - sp[n][0] * vy;
                }
                u[0] = s0 + bpk[0]; u[1] = s1 + bpk[1]; u[2] = s2 + bpk[2];
                u[3] = s3 + bpk[3]; u[4] = s4 + bpk[4]; u[5] = s5 + bpk[5];
            };

            // FISTA state.  x lives in two buffers (xa/xb, A-images ra/rb) whose roles swap every
            // iteration, so "x_k = x_k_1" (fista.cpp:37) costs no register moves.
            R xa[NF], xb[NF], y[NF], ra[6], rb[6], ry[6];
            if constexpr (CLDS) { UNROLL for (int j = 0; j < NF; ++j) { xa[j] = F0[j]; y[j] = xa[j]; } }
            else { UNROLL for (int j = 0; j < NF; ++j) { xa[j] = rvalid ? Fg[j] : R(0); y[j] = xa[j]; } }
            applyA(y, ry);
            UNROLL for (int k = 0; k < 6; ++k) ra[k] = ry[k];
            if constexpr (CLDS) { if (rvalid) { UNROLL for (int k = 0; k < 6; ++k) rec[18 + NF + k] = ry[k]; } }
            else
            if (XLDS && rvalid) { UNROLL for (int k = 0; k < 6; ++k) Rg[k] = ry[k]; }      // (x_0 itself is in the F block already)
            const R mu2 = mu * mu, imu = R(1) / (mu * mu + R(1));
            const double tol2 = tol * tol;
            R invL = R(2) * (R(1) / L_f);      // 2 / L, see above
            mask_t banded = 0;      // the fp32 step decisions (see BAND): all ones or 0 (a mask: a bool here would live in a vector register)
            float Llo = 0.0f, Lhi = 0.0f, flo = 0.0f, fhi = 0.0f;
            if constexpr (BAND) if (a.exact_step_decisions != 1) {
                bool wneg = false;
                UNROLL for (int j = 0; j < NF; ++j) wneg = wneg || wf[j] < R(0);
                banded = rho >= R(0) && __ballot(wneg) == 0 ? ~mask_t(0) : mask_t(0);
                band_L((double)L_f * 0.5, Llo, Lhi);
                band_u(floor2, flo, fhi);
            }
            // the lane-local screen of the certified loop (biconvex_lanes.h: screen_theta): a lane's own |d|^2 above theta settles the
            // iteration's floor and exit decisions for its problem without any sum; +inf (no lane is above it) unless the switch is 0.
            // Whatever `banded` says: squares are non-negative under any weights.
            [[maybe_unused]] double theta = __builtin_inf();
            if constexpr (BAND) if (a.exact_step_decisions == 0) theta = screen_theta(tol2, floor2);
            mask_t act = alive;
            // one FISTA iteration: reads x from xo/ro, leaves x_{k+1} in xn/rn, advances y/ry (XLDS: x_k from LDS, x_{k+1} to LDS;
            // the four arrays are then no more than the iteration's temporaries)
            auto iterate = [&](const R (&xo_reg)[NF], const R (&ro_reg)[6], R (&xn)[NF], R (&rn)[6], int i, auto certc) {
                constexpr bool CERT = decltype(certc)::value;      // the certified loop (see `cert`): no backtracking test unless |d| is tiny
                const R cm = (R)cmtab[i];
                R xo[NF], ro[6];
                if (!XLDS) {
                    UNROLL for (int j = 0; j < NF; ++j) xo[j] = xo_reg[j];
                    UNROLL for (int k = 0; k < 6; ++k) ro[k] = ro_reg[k];
                }
                mask_t done;
                mask_t pend = act;
                for (;;) {  // backtracking (fista.cpp:8-26); segments that accepted recompute the same values
                    // KQ: y of knots t - 1 and t + 1 (fetched per trial: nearly every step takes one, and held across the retry loop they
                    // would sit in accumulation registers)
                    [[maybe_unused]] R yp[KQ ? NF : 1], yn[KQ ? NF : 1];
                    if constexpr (KQ) {
                        shift_prev(y, yp);
                        shift_next(y, yn);
                        UNROLL for (int j = 0; j < NF; ++j) { yp[j] = keep_if(yp[j], fpm); yn[j] = keep_if(yn[j], fnm); }
                    }
                    // g/2 = Q y + q/2 + rho A^T (A y + bPk)          (problem.cpp:36-38,54-56), the step y - (2/L) g/2 and the
                    // "SoC" projection exactly as fista.cpp:52-70 writes it (zeroing by a 0 / 1 factor: one select per foot)
                    unsigned long long anycone = 0;     // lanes with a force on the cone branch, as a scalar mask
                    R fr[NF];
                    UNROLL for (int n = 0; n < E; ++n) {
                        const R zx = an[n] * ry[0] - sp[n][2] * ry[4] + sp[n][1] * ry[5];
                        const R zy = an[n] * ry[1] + sp[n][2] * ry[3] - sp[n][0] * ry[5];
                        const R zz = an[n] * ry[2] - sp[n][1] * ry[3] + sp[n][0] * ry[4];
                        R gx, gy, gz;
                        if constexpr (BQ) {      // rows 3n .. 3n + 2 of W y, added to rho A'(A y + bPk) column by column
                            gx = rho * zx; gy = rho * zy; gz = rho * zz;
                            UNROLL for (int j = 0; j < NF; ++j) {
                                gx = fmaR(Wb[sym_index(NF, 3 * n, j)], y[j], gx);
                                gy = fmaR(Wb[sym_index(NF, 3 * n + 1, j)], y[j], gy);
                                gz = fmaR(Wb[sym_index(NF, 3 * n + 2, j)], y[j], gz);
                            }
                        } else {
                            gx = fmaR(wf[3 * n], y[3 * n], rho * zx); gy = fmaR(wf[3 * n + 1], y[3 * n + 1], rho * zy);
                            gz = fmaR(wf[3 * n + 2], y[3 * n + 2], rho * zz);
                            if constexpr (KQ) {
                                gx = fmaR(ofp[3 * n], yp[3 * n], gx); gy = fmaR(ofp[3 * n + 1], yp[3 * n + 1], gy); gz = fmaR(ofp[3 * n + 2], yp[3 * n + 2], gz);
                                gx = fmaR(of[3 * n], yn[3 * n], gx); gy = fmaR(of[3 * n + 1], yn[3 * n + 1], gy); gz = fmaR(of[3 * n + 2], yn[3 * n + 2], gz);
                            }
                        }
                        if (HASQF) { gx += qf[3 * n]; gy += qf[3 * n + 1]; gz += qf[3 * n + 2]; }
                        fr[3 * n] = fmaR(-gx, invL, y[3 * n]);
                        fr[3 * n + 1] = fmaR(-gy, invL, y[3 * n + 1]);
                        fr[3 * n + 2] = fmaR(-gz, invL, y[3 * n + 2]);
                        if constexpr (FRAME) {     // the Euclidean projection about the contact's normal: fn along it, s2 = |f - fn n|^2
                            const R nx = nrm[3 * n], ny = nrm[3 * n + 1], nz = nrm[3 * n + 2];
                            const R fn = fmaR(nx, fr[3 * n], fmaR(ny, fr[3 * n + 1], nz * fr[3 * n + 2]));
                            const R tx = fmaR(-fn, nx, fr[3 * n]), ty = fmaR(-fn, ny, fr[3 * n + 1]), tz = fmaR(-fn, nz, fr[3 * n + 2]);
                            const R s2 = fmaR(tx, tx, fmaR(tz, tz, ty * ty));
                            const R m2 = muf[n] * muf[n], z2 = fn * fn;
                            const bool zero = fn <= R(0) && m2 * s2 <= z2;      // (the polar cone; wins at the origin)
                            const bool inside = fn >= R(0) && s2 <= m2 * z2;
                            anycone |= __ballot(!zero && !inside);
                            const R keep = zero ? R(0) : R(1);
                            xn[3 * n] = keep * fr[3 * n];
                            xn[3 * n + 1] = keep * fr[3 * n + 1];
                            xn[3 * n + 2] = keep * fr[3 * n + 2];
                            continue;
                        }
                        const R s = fmaR(fr[3 * n], fr[3 * n], fr[3 * n + 1] * fr[3 * n + 1]);
                        const R fz = fr[3 * n + 2];
                        if constexpr (CONE) {      // the Euclidean projection: origin, unchanged, or (below) the cone's surface
                            const R m2 = muf[n] * muf[n], z2 = fz * fz;
                            const bool zero = fz <= R(0) && m2 * s <= z2;      // (the polar cone; wins at the origin)
                            const bool inside = fz >= R(0) && s <= m2 * z2;
                            anycone |= __ballot(!zero && !inside);
                            const R keep = zero ? R(0) : R(1);
                            xn[3 * n] = keep * fr[3 * n];
                            xn[3 * n + 1] = keep * fr[3 * n + 1];
                            xn[3 * n + 2] = keep * fz;
                        } else {
                        const bool zero = (s * mu < -fz) || (fz < 0);
                        anycone |= __ballot(!zero && (s > mu * fz));
                        const R keep = zero ? R(0) : R(1);
                        xn[3 * n] = keep * fr[3 * n];
                        xn[3 * n + 1] = keep * fr[3 * n + 1];
                        xn[3 * n + 2] = keep * fz;
                        }
                    }
                    if constexpr (FRAME) {
                        if (anycone != 0) {   // a force outside both cones: onto the surface k ft + t n; skipped while no lane needs it
                            UNROLL for (int n = 0; n < E; ++n) {
                                const R nx = nrm[3 * n], ny = nrm[3 * n + 1], nz = nrm[3 * n + 2], mf = muf[n];
                                const R fn = fmaR(nx, fr[3 * n], fmaR(ny, fr[3 * n + 1], nz * fr[3 * n + 2]));
                                const R tx = fmaR(-fn, nx, fr[3 * n]), ty = fmaR(-fn, ny, fr[3 * n + 1]), tz = fmaR(-fn, nz, fr[3 * n + 2]);
                                const R s2 = fmaR(tx, tx, fmaR(tz, tz, ty * ty));
                                const R m2 = mf * mf, z2 = fn * fn;
                                const bool surf = !(fn <= R(0) && m2 * s2 <= z2) && !(fn >= R(0) && s2 <= m2 * z2);
                                const R s = sqrt(s2);
                                const R tn = fast_div(fmaR(mf, s, fn), m2 + R(1));
                                const R k = fast_div(mf * tn, s);      // (s > 0 on this branch: s2 = 0 is the origin or inside)
                                xn[3 * n] = surf ? fmaR(tn, nx, k * tx) : xn[3 * n];
                                xn[3 * n + 1] = surf ? fmaR(tn, ny, k * ty) : xn[3 * n + 1];
                                xn[3 * n + 2] = surf ? fmaR(tn, nz, k * tz) : xn[3 * n + 2];
                            }
                        }
                    } else
                    if constexpr (CONE) {
                        if (anycone != 0) {   // a force outside both cones: onto the surface; skipped while no lane needs it
                            UNROLL for (int n = 0; n < E; ++n) {
                                const R s2 = fmaR(fr[3 * n], fr[3 * n], fr[3 * n + 1] * fr[3 * n + 1]);
                                const R fz = fr[3 * n + 2], mf = muf[n];
                                const R m2 = mf * mf, z2 = fz * fz;
                                const bool surf = !(fz <= R(0) && m2 * s2 <= z2) && !(fz >= R(0) && s2 <= m2 * z2);
                                const R s = sqrt(s2);
                                const R tz = fast_div(fmaR(mf, s, fz), m2 + R(1));
                                const R k = fast_div(mf * tz, s);      // (s > 0 on this branch: s2 = 0 is the origin or inside)
                                xn[3 * n] = surf ? fr[3 * n] * k : xn[3 * n];
                                xn[3 * n + 1] = surf ? fr[3 * n + 1] * k : xn[3 * n + 1];
                                xn[3 * n + 2] = surf ? tz : xn[3 * n + 2];
                            }
                        }
                    } else
                    if (anycone != 0) {   // cone branch (fista.cpp:64-68); skipped while no lane needs it
                        UNROLL for (int n = 0; n < E; ++n) {
                            const R s = fmaR(fr[3 * n], fr[3 * n], fr[3 * n + 1] * fr[3 * n + 1]);
                            const R fz = fr[3 * n + 2];
                            const bool zero = (s * mu < -fz) || (fz < 0);
                            const bool cone = !zero && (s > mu * fz);
                            const R k = fast_div(fmaR(mu2, s, mu * fz), (mu2 + R(1)) * s);
                            xn[3 * n] = cone ? fr[3 * n] * k : xn[3 * n];
                            xn[3 * n + 1] = cone ? fr[3 * n + 1] * k : xn[3 * n + 1];
                            xn[3 * n + 2] = cone ? fmaR(mu, s, fz) * imu : xn[3 * n + 2];
                        }
                    }
                    applyA(xn, rn);
                    R g2 = 0, cv = 0, e2 = 0, dv[NF];
                    if (CERT) {
                        if constexpr (BAND) {}      // (the headline kernel's certified loop: in the screen below, and only where stage 1 misses)
                        else { UNROLL for (int j = 0; j < NF; ++j) { const R d = xn[j] - y[j]; g2 = fmaR(d, d, g2); } }
                    } else {
                    UNROLL for (int j = 0; j < NF; ++j) {
                        const R d = xn[j] - y[j];
                        dv[j] = d;
                        g2 = fmaR(d, d, g2);
                        if constexpr (!BQ) cv = fmaR(wf[j] * d, d, cv);
                    }
                    if constexpr (KQ) {      // the pairs (t, t + 1): 2 off_t d_t d_{t+1}, summed on their own so that ONE keep_if removes what came
                        R dn[NF], cp = 0;    // across the end of the segment
                        shift_next(dv, dn);
                        UNROLL for (int j = 0; j < NF; ++j) cp = fmaR((of[j] + of[j]) * dv[j], dn[j], cp);
                        cv += keep_if(cp, fnm);
                    }
                    if constexpr (BQ) {      // d'W d, row by row
                        UNROLL for (int r = 0; r < NF; ++r) {
                            R wd = Wb[sym_index(NF, r, 0)] * dv[0];
                            UNROLL for (int j = 1; j < NF; ++j) wd = fmaR(Wb[sym_index(NF, r, j)], dv[j], wd);
                            cv = fmaR(wd, dv[r], cv);
                        }
                    }
                    if (sizeof(R) == sizeof(double)) {
                        UNROLL for (int k = 0; k < 6; ++k) { const R e = rn[k] - ry[k]; e2 = fmaR(e, e, e2); }
                    } else {
                        // fp32: A d = (A y+ + bPk) - (A y + bPk) by subtraction carries the rounding of the two images (1e-7 of
                        // |A y|, whatever |d| is); near convergence rho |noise|^2 then exceeds (L/2)|d|^2 and the test retries
                        // for ever (L_f x 1.5 until it overflows: seen on ~1.5 % of the trot problems).  A applied to d itself
                        // has the rounding of |A d|.
                        R s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0;
                        UNROLL for (int n = 0; n < E; ++n) {
                            const R vx = dv[3 * n], vy = dv[3 * n + 1], vz = dv[3 * n + 2];
                            s0 += an[n] * vx; s1 += an[n] * vy; s2 += an[n] * vz;
                            s3 += sp[n][2] * vy - sp[n][1] * vz;
                            s4 += sp[n][0] * vz - sp[n][2] * vx;
                            s5 += sp[n][1] * vx - sp[n][0] * vy;
                        }
                        e2 = s0 * s0 + s1 * s1 + s2 * s2 + s3 * s3 + s4 * s4 + s5 * s5;
                    }
                    cv = fmaR(rho, e2, cv);
                    }
                    if (XLDS) {     // x_k and its image come in while the sums are reduced (unconditional: lanes without a knot read zeros)
                        UNROLL for (int j = 0; j < NF; ++j) xo[j] = Fz[j];
                        UNROLL for (int k = 0; k < 6; ++k) ro[k] = RFz[k];
                    }
                    mask_t bt;
                    if constexpr (BAND) {      // (the other instantiations compile the code below the `else` alone, as before the shortcut)
                        bt = 0;      // (certified: cvs <= rhs whatever the step)
                        bool settled = false;      // the screen: every live problem has a lane above theta -- no hand-over, no exit, no sum
                        if constexpr (CERT) {
                            // Two stages.  Stage 1 asks it of s, an fma chain over a few of the lane's squares (kScreenTermsF): s > theta
                            // settles what the whole partial g2 > theta settles.  The exact sums are ordered (squares are non-negative, a
                            // subset's sum is at most the whole) and each chain rounds at most NF = 12 times, by at most 2^-53 relative
                            // where the result is normal and by at most 2^-1075 absolute where it is not -- 24 x 2^-1075 is 2^-70 of
                            // s > theta >= 2^-1000 -- hence g2 >= s (1 - 24 x 2^-53 - 2^-70) > s (1 - 2^-48); the segment sum S in any order
                            // is at least g2 (fl(a + b) >= max(a, b) for a, b >= 0); and theta carries (1 + 2^-40) over max(tol^2, floor2):
                            // S > max(tol^2, floor2) (1 + 2^-41), above the floor, above tol^2 and outside the 1e-14 edge band.  NaN
                            // elsewhere in the segment makes S NaN and the three comparisons false, as with one stage.  Only on a miss is
                            // g2 made, in the one-stage order (its bits), and asked the one-stage question; then the code as it stood.
                            // theta = +inf (switch 1 or 2) fails both stages.
                            R s = 0;
                            UNROLL for (int k = 0; k < (int)(sizeof(kScreenTermsF) / sizeof(int)); ++k) { const R d = xn[kScreenTermsF[k]] - y[kScreenTermsF[k]]; s = fmaR(d, d, s); }
                            settled = seg_covered<LPP>(__ballot(s > theta), act);
                            if (!settled) {
                                UNROLL for (int j = 0; j < NF; ++j) { const R d = xn[j] - y[j]; g2 = fmaR(d, d, g2); }
                                settled = seg_covered<LPP>(__ballot(g2 > theta), act);
                            }
                        }
                        if (settled) done = 0;
                        else {
                            mask_t unclear = ~mask_t(0);      // designated lanes of live problems whose fp32 decisions are not clear
                            if (banded != 0) {      // the fp32 decisions, if every live problem's are clear (see BAND)
                                float gf = (float)g2, cf = (float)cv;
                                if (CERT) seg_sum1_f32<LPP>(gf);
                                else seg_sum2_f32<LPP>(gf, cf);
                                const mask_t yes = CERT ? __ballot(gf < flo) : __ballot(cf > gf * Lhi);
                                const mask_t no = CERT ? __ballot(gf > fhi) : __ballot(cf < gf * Llo);
                                const mask_t dyes = __ballot(gf < t2lo), dno = __ballot(gf > t2hi);
                                const mask_t clear = (yes | no) & (dyes | dno) & __ballot(gf >= 1e-24f) & __ballot(gf <= 1e30f);
                                unclear = ~clear & seg_desig<LPP>() & act;
                                if (unclear == 0) {
                                    if (CERT && (seg_uniform<LPP>(yes & seg_desig<LPP>()) & act) != 0) return false;      // (see below)
                                    if (!CERT) bt = yes;
                                    done = dyes;
                                }
                            }
                            if (unclear != 0) {
                                double g2s = (double)g2, cvs = (double)cv;
                                if (CERT) {
                                    sum1(g2s);
                                    // a live problem's step below the floor: nothing of this iteration is kept, the tested loop runs it again
                                    if ((seg_uniform<LPP>(__ballot(g2s < floor2) & seg_desig<LPP>()) & act) != 0) return false;
                                } else sum2(g2s, cvs);
                                // fista.cpp:14-17: G = sqrt(g2); retry if cv > (L/2) G*G; done if G < tol.  G*G and g2
                                // differ by a few ulp, so outside a 1e-14 relative band the sqrt cannot change either
                                // decision; inside it the reference expression is evaluated as written.
                                const double Lh = (double)L_f * 0.5, rhs = Lh * g2s;
                                if (!CERT) bt = __ballot(cvs > rhs);
                                done = __ballot(g2s < tol2);
                                const mask_t edge = __ballot((!CERT && fabs(cvs - rhs) <= 1e-14 * rhs) || (fabs(g2s - tol2) <= 1e-14 * tol2)) & seg_desig<LPP>();
                                if (edge != 0) {
                                    const double Gn = sqrt(g2s);
                                    if (!CERT) bt = __ballot(cvs > Lh * (Gn * Gn));
                                    done = __ballot(Gn < tol);
                                }
                            }
                        }
                    } else {
                        double g2s = (double)g2, cvs = (double)cv;
                        if (CERT) {
                            sum1(g2s);
                            // a live problem's step below the floor: nothing of this iteration is kept, the tested loop runs it again
                            if ((seg_uniform<LPP>(__ballot(g2s < floor2) & seg_desig<LPP>()) & act) != 0) return false;
                        } else sum2(g2s, cvs);
                        // fista.cpp:14-17: G = sqrt(g2); retry if cv > (L/2) G*G; done if G < tol.  G*G and g2
                        // differ by a few ulp, so outside a 1e-14 relative band the sqrt cannot change either
                        // decision; inside it the reference expression is evaluated as written.
                        const double Lh = (double)L_f * 0.5, rhs = Lh * g2s;
                        bt = CERT ? mask_t(0) : __ballot(cvs > rhs);      // (certified: cvs <= rhs whatever the step)
                        done = __ballot(g2s < tol2);
                        const mask_t edge = __ballot((!CERT && fabs(cvs - rhs) <= 1e-14 * rhs) || (fabs(g2s - tol2) <= 1e-14 * tol2)) & seg_desig<LPP>();
                        if (edge != 0) {
                            const double Gn = sqrt(g2s);
                            if (!CERT) bt = __ballot(cvs > Lh * (Gn * Gn));
                            done = __ballot(Gn < tol);
                        }
                    }
                    bt = seg_uniform<LPP>(bt);      // (LPP = 21: the sums live at three lanes; their decisions go to their segments)
                    done = seg_uniform<LPP>(done);
                    if (XLDS) {     // a use that stays in this loop: without it hipcc sinks the reads to the momentum step, where their latency shows
                        UNROLL for (int j = 0; j < NF; ++j) keep_here(xo[j]);
                        UNROLL for (int k = 0; k < 6; ++k) keep_here(ro[k]);
                    }
                    bt &= pend;
                    pend = bt;
                    if (bt == 0) break;
                    if (lanes(bt)) { L_f *= beta; ++bt_f; }
                    invL = R(2) * (R(1) / L_f);
                    if constexpr (BAND) if (banded != 0) band_L((double)L_f * 0.5, Llo, Lhi);
                }
                if (!XLDS) {
                    const mask_t last = act & (i == maxit - 1 ? ~mask_t(0) : done) & rvalid_m;
                    if (lanes(last)) { UNROLL for (int j = 0; j < NF; ++j) Fg[j] = xn[j]; }   // x_k of a finishing problem is latched
                }
                // momentum (fista.cpp:33-47); A-images follow by linearity
                // (the headline kernel's certified loop: fma3, no copies at the loop's end.  Nested conditions on purpose: `BAND && CERT`
                // depends on the lambda's own parameter, which makes the closure capture BAND -- and that moved the register allocation
                // of the block- and band-cost kernels)
                UNROLL for (int j = 0; j < NF; ++j) {
                    if constexpr (BAND) {
                        if constexpr (CERT) y[j] = fma3(cm, xn[j] - xo[j], xn[j]);
                        else y[j] = fmaR(cm, xn[j] - xo[j], xn[j]);
                    } else y[j] = fmaR(cm, xn[j] - xo[j], xn[j]);
                }
                UNROLL for (int k = 0; k < 6; ++k) ry[k] = fmaR(cm, rn[k] - ro[k], rn[k]);
                if (XLDS && lanes(act & rvalid_m)) {      // problems still iterating (a finished one keeps the x_k it finished with)
                    UNROLL for (int j = 0; j < NF; ++j) Fg[j] = xn[j];
                    UNROLL for (int k = 0; k < 6; ++k) Rg[k] = rn[k];
                }
                it_f += lanes(act) ? 1 : 0;
                act &= ~done;
                return true;
            };
            // the certified loop, if the phase has its certificate, then the tested one from the iteration the first left undone (the
            // last maxit: none); iteration i reads x_k from xa when i is even, so an odd start first moves x_k there
            auto loop = [&](int i0, auto certc) {
                for (int i = i0; i < maxit; i += 2) {
                    if (act == 0) break;
                    if (!iterate(xa, ra, xb, rb, i, certc)) return i;
                    if (i + 1 >= maxit || act == 0) break;
                    if (!iterate(xb, rb, xa, ra, i + 1, certc)) return i + 1;
                }
                return maxit;
            };
            int i0 = 0;
            if constexpr (CLDS) {
                // CLDS: the certified loop with F_k and its image in registers (xa / ra and xb / rb, roles alternating) and 18 of the
                // phase's constants -- the weights and bPk -- in LDS, as in the motion step (described there; the area is the same, the
                // phases exclusive).  A lambda of its own: the shared `iterate` stays what every other kernel compiles.  Its certified
                // trial, operation for operation: gradient, step, "SoC" projection, image, screen, the fp32 or fp64 decisions, momentum.
                // A lane without a force knot reads zeros for its weights and bPk, which is what they are; its values stay zeros.
                // The F / R blocks are written where they are read again: at a problem's `done` bit or at maxit - 1 (F_{k+1} and its
                // image), and F_k and its image of the problems still iterating in front of a hand-over.  Lane-local stores under the
                // lane's own problem's mask, as the shared loop's: a diverged wave-mate's NaNs stay its own.
                if (cert) {
                    const unsigned cb = consts_offset(rvalid_m);
                    auto consts = [&]() { return reinterpret_cast<R *>(reinterpret_cast<char *>(lds_raw) + opaque_copy(cb)); };
                    if (rvalid) { R *Cg = consts(); UNROLL for (int j = 0; j < NF; ++j) Cg[j] = wf[j]; UNROLL for (int k = 0; k < 6; ++k) Cg[NF + k] = bpk[k]; }
                    park_f();      // (the step constant and the counters rest in the header across the loop, as across the motion step)
                    R wc[NF];
                    { const R *Cz = consts(); UNROLL for (int j = 0; j < NF; ++j) wc[j] = Cz[j]; }
                    // (the scalar side of the loop -- counts from the exit index, `act` and the screen's words changed only where `done`
                    // has a bit, the last iteration's store at the loop's exits, a scalar momentum coefficient, the return value that says
                    // how the loop goes on: described at the motion step's loop)
                    int c0 = 0, c1 = 0;      // iterations of the wave's two problems that have left the loop (scalar registers)
                    unsigned dead0, dead1;
                    seg_dead32(act, dead0, dead1);
                    R cmn = uniform_load(cmtab, 0u);
                    auto store_fr = [&](mask_t m, const R (&xv)[NF], const R (&rv)[6]) {
                        if (lanes(m & rvalid_m)) {
                            R *Xs = knot_record();
                            UNROLL for (int j = 0; j < NF; ++j) Xs[18 + j] = xv[j];
                            UNROLL for (int k = 0; k < 6; ++k) Xs[18 + NF + k] = rv[k];
                        }
                    };
                    constexpr int kGo = 0, kHandOver = 1, kAllLeft = 2;
                    // an iteration that the screen does not settle: the step decisions from the sums, a hand-over, or problems that finish
                    auto unsettled = [&](const R (&xo)[NF], const R (&ro)[6], const R (&xn)[NF], const R (&rn)[6], int i, R g2) -> int {
                        mask_t done = 0;
                        mask_t unclear = ~mask_t(0);      // designated lanes of live problems whose fp32 decisions are not clear
                        if (banded != 0) {      // the fp32 decisions, if every live problem's are clear (see BAND)
                            float gf = (float)g2;
                            seg_sum1_f32<LPP>(gf);
                            const mask_t yes = __ballot(gf < flo), no = __ballot(gf > fhi);
                            const mask_t dyes = __ballot(gf < t2lo), dno = __ballot(gf > t2hi);
                            const mask_t clear = (yes | no) & (dyes | dno) & __ballot(gf >= 1e-24f) & __ballot(gf <= 1e30f);
                            unclear = ~clear & act;
                            if (unclear == 0) {
                                if ((yes & act) != 0) { store_fr(act, xo, ro); return kHandOver; }
                                done = dyes;
                            }
                        }
                        if (unclear != 0) {
                            double g2s = (double)g2;
                            sum1(g2s);
                            // a live problem's step below the floor: nothing of this iteration is kept, the tested loop runs it again
                            if ((__ballot(g2s < floor2) & act) != 0) { store_fr(act, xo, ro); return kHandOver; }
                            done = __ballot(g2s < tol2);      // (see the shared loop for the sqrt-free form)
                            if (__ballot(fabs(g2s - tol2) <= 1e-14 * tol2) != 0) done = __ballot(sqrt(g2s) < tol);
                        }
                        const mask_t latch = act & done;
                        if (latch != 0) {      // problems that finish here: F_{k+1} and its image, their counts, and what follows from `act`
                            store_fr(latch, xn, rn);
                            if ((unsigned)latch != 0u) c0 = i + 1;
                            if ((unsigned)(latch >> 32) != 0u) c1 = i + 1;
                            act &= ~done;
                            if (act == 0) return kAllLeft;      // (nothing reads y behind the loop)
                            seg_dead32(act, dead0, dead1);
                        }
                        return kGo;
                    };
                    auto iterate_k = [&](const R (&xo)[NF], const R (&ro)[6], R (&xn)[NF], R (&rn)[6], int i) -> int {
                        const R cm = cmn;
                        cmn = uniform_load(cmtab, min((unsigned)i + 1u, (unsigned)kMaxFistaIters - 1u));      // (the next iteration's)
                        unsigned long long anycone = 0;     // lanes with a force on the cone branch, as a scalar mask
                        R fr[NF];
                        UNROLL for (int n = 0; n < E; ++n) {
                            const R zx = an[n] * ry[0] - sp[n][2] * ry[4] + sp[n][1] * ry[5];
                            const R zy = an[n] * ry[1] + sp[n][2] * ry[3] - sp[n][0] * ry[5];
                            const R zz = an[n] * ry[2] - sp[n][1] * ry[3] + sp[n][0] * ry[4];
                            R gx, gy, gz;
                            gx = fmaR(wc[3 * n], y[3 * n], rho * zx); gy = fmaR(wc[3 * n + 1], y[3 * n + 1], rho * zy);
                            gz = fmaR(wc[3 * n + 2], y[3 * n + 2], rho * zz);
                            fr[3 * n] = fmaR(-gx, invL, y[3 * n]);
                            fr[3 * n + 1] = fmaR(-gy, invL, y[3 * n + 1]);
                            fr[3 * n + 2] = fmaR(-gz, invL, y[3 * n + 2]);
                            const R s = fmaR(fr[3 * n], fr[3 * n], fr[3 * n + 1] * fr[3 * n + 1]);
                            const R fz = fr[3 * n + 2];
                            const bool zero = (s * mu < -fz) || (fz < 0);
                            anycone |= __ballot(!zero && (s > mu * fz));
                            const R keep = zero ? R(0) : R(1);
                            xn[3 * n] = keep * fr[3 * n];
                            xn[3 * n + 1] = keep * fr[3 * n + 1];
                            xn[3 * n + 2] = keep * fz;
                        }
                        if (anycone != 0) {   // cone branch (fista.cpp:64-68); skipped while no lane needs it
                            UNROLL for (int n = 0; n < E; ++n) {
                                const R s = fmaR(fr[3 * n], fr[3 * n], fr[3 * n + 1] * fr[3 * n + 1]);
                                const R fz = fr[3 * n + 2];
                                const bool zero = (s * mu < -fz) || (fz < 0);
                                const bool cone = !zero && (s > mu * fz);
                                const R k = fast_div(fmaR(mu2, s, mu * fz), (mu2 + R(1)) * s);
                                xn[3 * n] = cone ? fr[3 * n] * k : xn[3 * n];
                                xn[3 * n + 1] = cone ? fr[3 * n + 1] * k : xn[3 * n + 1];
                                xn[3 * n + 2] = cone ? fmaR(mu, s, fz) * imu : xn[3 * n + 2];
                            }
                        }
                        {   // applyA, its bPk read behind the projection and used last, behind one wait for all six
                            R bk[6];
                            const R *Cz = reinterpret_cast<const R *>(reinterpret_cast<const char *>(lds_raw) + opaque_copy_after(cb, xn[NF - 1]));
                            UNROLL for (int k = 0; k < 6; ++k) bk[k] = Cz[NF + k];
                            R s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0;
                            UNROLL for (int n = 0; n < E; ++n) {
                                const R vx = xn[3 * n], vy = xn[3 * n + 1], vz = xn[3 * n + 2];
                                s0 += an[n] * vx; s1 += an[n] * vy; s2 += an[n] * vz;
                                s3 += sp[n][2] * vy - sp[n][1] * vz;
                                s4 += sp[n][0] * vz - sp[n][2] * vx;
                                s5 += sp[n][1] * vx - sp[n][0] * vy;
                            }
                            keep_here(bk);
                            rn[0] = s0 + bk[0]; rn[1] = s1 + bk[1]; rn[2] = s2 + bk[2];
                            rn[3] = s3 + bk[3]; rn[4] = s4 + bk[4]; rn[5] = s5 + bk[5];
                        }
                        {   // the two-stage screen (see the shared loop), as nested branches (see the motion step's loop)
                            R s = 0;
                            UNROLL for (int k = 0; k < (int)(sizeof(kScreenTermsF) / sizeof(int)); ++k) { const R d = xn[kScreenTermsF[k]] - y[kScreenTermsF[k]]; s = fmaR(d, d, s); }
                            if (!seg_covered32(__ballot(s > theta), dead0, dead1)) {
                                R g2 = 0;
                                UNROLL for (int j = 0; j < NF; ++j) { const R d = xn[j] - y[j]; g2 = fmaR(d, d, g2); }
                                const mask_t own = __ballot(g2 > theta);
                                if (!seg_covered32(own, dead0, dead1) && !seg_covered32(own | quad_screen(g2, theta), dead0, dead1)) {      // (the quad stage: biconvex_lanes.h)
                                    const int r = unsettled(xo, ro, xn, rn, i, g2);
                                    if (r != kGo) return r;
                                }
                            }
                        }
                        { const R *Cz = consts(); UNROLL for (int j = 0; j < NF; ++j) wc[j] = Cz[j]; }      // (the next iteration's)
                        UNROLL for (int j = 0; j < NF; ++j) y[j] = fma3_s(cm, xn[j] - xo[j], xn[j]);
                        UNROLL for (int k = 0; k < 6; ++k) ry[k] = fmaR(cm, rn[k] - ro[k], rn[k]);
                        keep_here(wc);      // (a use that stays here: the loads are not sunk to the gradient step; one statement, one wait)
                        return kGo;
                    };
                    // Two feet per lane ("Force loop: two feet per lane").  A swing foot -- an = sp = 0, F_0 = +0 -- stays +0
                    // through every operation of the loop above and adds +0 to every sum.  Here the 32 lanes of a segment are re-mapped onto
                    // UNITS: a knot, a rank and up to two of the knot's contact feet in foot order (slots); a knot with three or four contacts
                    // takes a second unit on the lane behind its first.  Per slot the operations of iterate_k on the same operands; the six
                    // image sums are chains over the feet in foot order, so the knot's first unit starts them from +0, hands its partial sums
                    // to the second unit (shift_prev), which continues them with its slots and hands the finished sums back (shift_next).
                    // Wave-uniform eligibility: the switch, at most 32 units per problem, every swing foot's F_0 the bits of +0.0.  A `done`
                    // latch and the exit by maxit store F_{k+1} (every unit its own feet) and its image (the knot's first unit); a step
                    // below the floor or a non-finite value at an exit stores nothing of the problems still iterating and falls through to
                    // the loop above, which runs the phase from iteration 0 (the records still hold F_0 and its image).
                    bool pairs_done = false;
                    if ((MATES ? (a.force_foot_pairs & 1) : a.force_foot_pairs) != 0 && act != 0 && maxit > 0) {
                        keep_here(xa);      // (F_0's bits are looked at here: made in the prologue, the partial results are parked in scratch memory)
                        // what the phase itself has to show: every swing foot's F_0 the bits of +0.0, and the feet without contact in the
                        // plan (an = 0: the map's rule) swing feet in this phase's values too -- a non-finite X makes their sp NaN, and
                        // the wave then runs four feet per lane, where such a foot's NaNs go the way they always went
                        unsigned f0bits = 0;      // the swing feet's F_0, every bit or'ed: +0.0 is no bit
                        bool stale = false;
                        UNROLL for (int n = 0; n < E; ++n) {
                            const bool off = an[n] == R(0);
                            const bool swing = off && sp[n][0] == R(0) && sp[n][1] == R(0) && sp[n][2] == R(0);
                            stale = stale || (off && !swing);
                            unsigned w = 0;
                            UNROLL for (int k = 0; k < 3; ++k) w |= (unsigned)__double2hiint((double)xa[3 * n + k]) | (unsigned)__double2loint((double)xa[3 * n + k]);
                            f0bits |= swing ? w : 0u;
                        }
                        const bool f0ok = f0bits == 0u && !stale;
                        if (pair_fits && __ballot(!f0ok) == 0) {
                            #pragma clang fp contract(off)
                            // ---- the lane's entry of the unit map (made in front of the ADMM loop: unit_map)
                            const unsigned e = unit_map()[opaque_copy(lane_id()) & 31u];
                            lds_fence();
                            const bool uval = (e & 0x8000u) == 0u;
                            const int mrank = (e & 32u) != 0u ? -1 : 0;
                            const mask_t tfirst_m = __ballot(uval && mrank == 0 && __popc((e >> 8) & 15u) > 2);      // the first units of knots with two (a mask: see `lanes`)
                            unsigned fs[2]; bool sv[2];
                            {
                                unsigned um = uval ? (e >> 8) & 15u : 0u;
                                if (mrank != 0) { um &= um - 1u; um &= um - 1u; }
                                sv[0] = um != 0u; fs[0] = sv[0] ? (unsigned)__builtin_ctz(um) : 0u; um &= um - 1u;
                                sv[1] = um != 0u; fs[1] = sv[1] ? (unsigned)__builtin_ctz(um) : 0u;
                            }
                            // addresses, as byte offsets into LDS: the knot's record (its X block) and its constants; what a unit does not
                            // have it reads from the zeros at the front (element lane mod 32 onward: at most 31 + 5 < kLdsZeros)
                            const unsigned lnu = opaque_copy(lane_id());
                            const unsigned zoff = 8u * (lnu & 31u);
                            const unsigned urec = 8u * ((unsigned)(kLdsZeros + kSegLds) + lnu / 32u * (unsigned)(kSegLds + (H + 1) * KL) + (e & 31u) * (unsigned)KL);
                            const unsigned ucon = 8u * ((unsigned)(kLdsZeros + 2 * (kSegLds + (H + 1) * KL)) + (lnu / 32u * (unsigned)(H + 1) + (e & 31u)) * (unsigned)kLoopConstLds);
                            auto ldsp = [&](unsigned off) { return reinterpret_cast<R *>(reinterpret_cast<char *>(lds_raw) + opaque_copy(off)); };
                            const unsigned cbk = uval ? ucon + 8u * (unsigned)NF : zoff;
                            const unsigned cbs[2] = {sv[0] ? ucon + 24u * fs[0] : zoff, sv[1] ? ucon + 24u * fs[1] : zoff};
                            // an, sp of the slots: the prologue's expressions on the knot's c, r, X[0..2], dt
                            R pan[2], psp[2][3], py[6], pxa[6], pxb[6], pra[6], prb[6], pry[6], pwc[6];
                            {
                                const unsigned oKu = 8u * (sl_ * (unsigned)H + (uval ? e & 31u : 0u));
                                const R dtu = ldz<R>(a.dt + wave0 * H, oKu, 0, uval);
                                R Xu3[3];
                                { const R *Xr = ldsp(uval ? urec : zoff); UNROLL for (int k = 0; k < 3; ++k) Xu3[k] = Xr[k]; }
                                UNROLL for (int s = 0; s < 2; ++s) {
                                    const unsigned oCu = oKu * (unsigned)(E * 4) + 32u * fs[s];
                                    const R cu = ldz<R>(cnt_u, oCu, 0, sv[s]);
                                    const R av = cu * (dtu / m);
                                    pan[s] = sv[s] ? av : R(0);
                                    UNROLL for (int k = 0; k < 3; ++k) {
                                        const R ru = ldz<R>(cnt_u, oCu, 1 + k, sv[s]);
                                        const R v = cu * (Xu3[k] - ru) * dtu;
                                        psp[s][k] = sv[s] ? v : R(0);
                                    }
                                    const R *Fr = ldsp(sv[s] ? urec + 8u * 18u + 24u * fs[s] : zoff);
                                    const R *Cs = ldsp(cbs[s]);
                                    UNROLL for (int k = 0; k < 3; ++k) { pxa[3 * s + k] = Fr[k]; py[3 * s + k] = pxa[3 * s + k]; pwc[3 * s + k] = Cs[k]; }
                                }
                                const R *Rr = ldsp(uval ? urec + 8u * (unsigned)(18 + NF) : zoff);
                                UNROLL for (int k = 0; k < 6; ++k) { pry[k] = Rr[k]; pra[k] = pry[k]; }
                            }
                            constexpr int kReplay = 3;
                            // an exit: F_{k+1} and its image of the problems in m to their knots' records -- unless one of them holds a
                            // non-finite value (false: nothing is stored, the phase is run again by the loop above)
                            auto store_p = [&](mask_t m, const R (&xv)[6], const R (&rv)[6]) -> bool {
                                bool bad = false;
                                UNROLL for (int j = 0; j < 6; ++j) bad = bad || !(__builtin_fabs((double)xv[j]) < __builtin_inf()) || !(__builtin_fabs((double)rv[j]) < __builtin_inf());
                                if ((__ballot(bad) & m) != 0) return false;
                                if (lanes(m) && uval) {
                                    R *Xs = ldsp(urec);
                                    UNROLL for (int s = 0; s < 2; ++s) {
                                        if (sv[s]) { R *Fs = Xs + 18 + 3 * fs[s]; UNROLL for (int k = 0; k < 3; ++k) Fs[k] = xv[3 * s + k]; }
                                    }
                                    if (mrank == 0) { UNROLL for (int k = 0; k < 6; ++k) Xs[18 + NF + k] = rv[k]; }
                                }
                                return true;
                            };
                            // an iteration that the screen does not settle: the knot's |d|^2 in the four-foot order (the first unit's chain,
                            // continued by the second), brought to the knot's lane; from there the sums and decisions of `unsettled`
                            auto unsettled_p = [&](const R (&xn)[6], const R (&rn)[6], int i, R g2own) -> int {
                                R g2;
                                {
                                    const R gin = keep_if(from_prev(g2own), mrank);
                                    R g = gin;
                                    UNROLL for (int j = 0; j < 6; ++j) { const R d = xn[j] - py[j]; g = fmaR(d, d, g); }
                                    const unsigned ln = opaque_copy(lane_id()), tl = ln & 31u;
                                    const unsigned tw = reinterpret_cast<const unsigned *>(unit_map())[16];      // (the segment's knots with two units)
                                    const unsigned last = tl + (unsigned)__popc(tw & ((2u << tl) - 1u));      // the knot's last unit
                                    const int src = (int)(4u * ((ln & 32u) + (last & 31u)));
                                    const double gd = (double)g;
                                    const int lo = __builtin_amdgcn_ds_bpermute(src, __double2loint(gd)), hi = __builtin_amdgcn_ds_bpermute(src, __double2hiint(gd));
                                    g2 = rvalid ? (R)__hiloint2double(hi, lo) : R(0);
                                }
                                mask_t done = 0;
                                mask_t unclear = ~mask_t(0);
                                if (banded != 0) {
                                    float gf = (float)g2;
                                    seg_sum1_f32<LPP>(gf);
                                    const mask_t yes = __ballot(gf < flo), no = __ballot(gf > fhi);
                                    const mask_t dyes = __ballot(gf < t2lo), dno = __ballot(gf > t2hi);
                                    const mask_t clear = (yes | no) & (dyes | dno) & __ballot(gf >= 1e-24f) & __ballot(gf <= 1e30f);
                                    unclear = ~clear & act;
                                    if (unclear == 0) {
                                        if ((yes & act) != 0) return kReplay;
                                        done = dyes;
                                    }
                                }
                                if (unclear != 0) {
                                    double g2s = (double)g2;
                                    sum1(g2s);
                                    if ((__ballot(g2s < floor2) & act) != 0) return kReplay;
                                    done = __ballot(g2s < tol2);
                                    if (__ballot(fabs(g2s - tol2) <= 1e-14 * tol2) != 0) done = __ballot(sqrt(g2s) < tol);
                                }
                                const mask_t latch = act & done;
                                if (latch != 0) {
                                    if (!store_p(latch, xn, rn)) return kReplay;
                                    if ((unsigned)latch != 0u) c0 = i + 1;
                                    if ((unsigned)(latch >> 32) != 0u) c1 = i + 1;
                                    act &= ~done;
                                    if (act == 0) return kAllLeft;
                                    seg_dead32(act, dead0, dead1);
                                }
                                return kGo;
                            };
                            auto iterate_p = [&](const R (&xo)[6], const R (&ro)[6], R (&xn)[6], R (&rn)[6], int i) -> int {
                                #pragma clang fp contract(off)
                                const R cm = cmn;
                                cmn = uniform_load(cmtab, min((unsigned)i + 1u, (unsigned)kMaxFistaIters - 1u));
                                unsigned long long anycone = 0;
                                R fr[6];
                                UNROLL for (int s = 0; s < 2; ++s) {      // (iterate_k's gradient, step and projection, with its contractions spelled out)
                                    const R zx = fmaR(psp[s][1], pry[5], fmaR(pan[s], pry[0], -(psp[s][2] * pry[4])));
                                    const R zy = fmaR(-psp[s][0], pry[5], fmaR(pan[s], pry[1], psp[s][2] * pry[3]));
                                    const R zz = fmaR(psp[s][0], pry[4], fmaR(pan[s], pry[2], -(psp[s][1] * pry[3])));
                                    const R gx = fmaR(pwc[3 * s], py[3 * s], rho * zx), gy = fmaR(pwc[3 * s + 1], py[3 * s + 1], rho * zy);
                                    const R gz = fmaR(pwc[3 * s + 2], py[3 * s + 2], rho * zz);
                                    fr[3 * s] = fmaR(-gx, invL, py[3 * s]);
                                    fr[3 * s + 1] = fmaR(-gy, invL, py[3 * s + 1]);
                                    fr[3 * s + 2] = fmaR(-gz, invL, py[3 * s + 2]);
                                    const R sq = fmaR(fr[3 * s], fr[3 * s], fr[3 * s + 1] * fr[3 * s + 1]);
                                    const R fz = fr[3 * s + 2];
                                    const bool zero = (sq * mu < -fz) || (fz < 0);
                                    anycone |= __ballot(!zero && (sq > mu * fz));
                                    const R keep = zero ? R(0) : R(1);
                                    xn[3 * s] = keep * fr[3 * s];
                                    xn[3 * s + 1] = keep * fr[3 * s + 1];
                                    xn[3 * s + 2] = keep * fz;
                                }
                                if (anycone != 0) {
                                    UNROLL for (int s = 0; s < 2; ++s) {
                                        const R sq = fmaR(fr[3 * s], fr[3 * s], fr[3 * s + 1] * fr[3 * s + 1]);
                                        const R fz = fr[3 * s + 2];
                                        const bool zero = (sq * mu < -fz) || (fz < 0);
                                        const bool cone = !zero && (sq > mu * fz);
                                        const R k = fast_div(fmaR(mu2, sq, mu * fz), (mu2 + R(1)) * sq);
                                        xn[3 * s] = cone ? fr[3 * s] * k : xn[3 * s];
                                        xn[3 * s + 1] = cone ? fr[3 * s + 1] * k : xn[3 * s + 1];
                                        xn[3 * s + 2] = cone ? fmaR(mu, sq, fz) * imu : xn[3 * s + 2];
                                    }
                                }
                                {   // the image: the cross products once, the chains twice (from +0, and from the knot's first unit's partial sums)
                                    R bk[6];
                                    const R *Cz = reinterpret_cast<const R *>(reinterpret_cast<const char *>(lds_raw) + opaque_copy_after(cbk, xn[5]));
                                    UNROLL for (int k = 0; k < 6; ++k) bk[k] = Cz[k];
                                    R u[2][3];
                                    UNROLL for (int s = 0; s < 2; ++s) {
                                        const R vx = xn[3 * s], vy = xn[3 * s + 1], vz = xn[3 * s + 2];
                                        u[s][0] = fmaR(psp[s][2], vy, -(psp[s][1] * vz));
                                        u[s][1] = fmaR(psp[s][0], vz, -(psp[s][2] * vx));
                                        u[s][2] = fmaR(psp[s][1], vx, -(psp[s][0] * vy));
                                    }
                                    auto chain = [&](const R (&in)[6], R (&o)[6]) {
                                        UNROLL for (int k = 0; k < 6; ++k) o[k] = in[k];
                                        UNROLL for (int s = 0; s < 2; ++s) {
                                            UNROLL for (int k = 0; k < 3; ++k) { o[k] = fmaR(pan[s], xn[3 * s + k], o[k]); o[3 + k] = o[3 + k] + u[s][k]; }
                                        }
                                    };
                                    const R z6[6] = {0, 0, 0, 0, 0, 0};
                                    R p[6], pin[6], q[6], back[6];
                                    chain(z6, p);
                                    shift_prev(p, pin);
                                    UNROLL for (int k = 0; k < 6; ++k) pin[k] = keep_if(pin[k], mrank);
                                    chain(pin, q);
                                    shift_next(q, back);
                                    keep_here(bk);
                                    UNROLL for (int k = 0; k < 6; ++k) rn[k] = (lanes(tfirst_m) ? back[k] : q[k]) + bk[k];
                                }
                                {   // the two-stage screen, on the lane's own slots: a partial over fewer terms can only miss more often
                                    const R d2 = xn[2] - py[2];
                                    const R sc = fmaR(d2, d2, R(0));
                                    if (!seg_covered32(__ballot(sc > theta), dead0, dead1)) {
                                        R g2 = 0;
                                        UNROLL for (int j = 0; j < 6; ++j) { const R d = xn[j] - py[j]; g2 = fmaR(d, d, g2); }
                                        const mask_t own = __ballot(g2 > theta);
                                        if (!seg_covered32(own, dead0, dead1) && !seg_covered32(own | quad_screen(g2, theta), dead0, dead1)) {      // (a quad of units: as sound)
                                            const int r = unsettled_p(xn, rn, i, g2);
                                            if (r != kGo) return r;
                                        }
                                    }
                                }
                                { UNROLL for (int s = 0; s < 2; ++s) { const R *Cs = ldsp(cbs[s]); UNROLL for (int k = 0; k < 3; ++k) pwc[3 * s + k] = Cs[k]; } }
                                UNROLL for (int j = 0; j < 6; ++j) py[j] = fma3_s(cm, xn[j] - xo[j], xn[j]);
                                UNROLL for (int k = 0; k < 6; ++k) pry[k] = fmaR(cm, rn[k] - ro[k], rn[k]);
                                keep_here(pwc);
                                return kGo;
                            };
                            int pr = kGo;
                            bool stored = true;
                            for (int i = 0;;) {
                                pr = iterate_p(pxa, pra, pxb, prb, i);
                                if (pr != kGo) break;
                                if (i + 1 >= maxit) { stored = store_p(act, pxb, prb); break; }
                                pr = iterate_p(pxb, prb, pxa, pra, i + 1);
                                if (pr != kGo) break;
                                i += 2;
                                if (i >= maxit) { stored = store_p(act, pxa, pra); break; }
                            }
                            lds_fence();
                            if (pr == kReplay || !stored) {
                                // the phase again, by the loop below: F_0 and its image from the records, the first weights and coefficient
                                // (and the knot's an / sp, made again from the plan by the prologue's expressions: held across the loop above
                                // they are 32 registers, which that loop then finds in scratch memory)
                                R *rr = record_or_front(kvalid_m);
                                {
                                    const unsigned ph2 = opaque_zero();
                                    const unsigned oC2 = make_off(opaque_copy(sl)).K * (unsigned)(E * 4) + ph2;
                                    R X3[3];
                                    UNROLL for (int k = 0; k < 3; ++k) { const R v = rr[k]; X3[k] = kvalid ? v : R(0); }
                                    UNROLL for (int n = 0; n < E; ++n) {
                                        const R cn = ldz<R>(cnt_u, oC2, 4 * n, rvalid);
                                        an[n] = cn * (dt / m);
                                        UNROLL for (int k = 0; k < 3; ++k) sp[n][k] = cn * (X3[k] - ldz<R>(cnt_u, oC2, 4 * n + 1 + k, rvalid)) * dt;
                                    }
                                }
                                lds_block(rr + 18, xa, rvalid);
                                lds_block(rr + 18 + NF, ry, rvalid);
                                UNROLL for (int j = 0; j < NF; ++j) y[j] = xa[j];
                                UNROLL for (int k = 0; k < 6; ++k) ra[k] = ry[k];
                                { const R *Cz = consts(); UNROLL for (int j = 0; j < NF; ++j) wc[j] = Cz[j]; }
                                cmn = uniform_load(cmtab, 0u);
                                seg_dead32(act, dead0, dead1);
                            } else {
                                pairs_done = true;
                                if (l0 && lnu < 32u) atomicAdd(&g_foot_pair_phases, 1ull);
                                // (the phase is over -- neither loop below runs, i0 = maxit -- which hipcc does not see: it carried the
                                // four-foot loop's 126 registers of state through the loop above, whose own values then went to scratch
                                // memory.  Defined here, by no instruction, they are dead across it)
                                auto forget = [](R &v) { asm volatile("" : "=v"(v)); };
                                UNROLL for (int n = 0; n < E; ++n) { forget(an[n]); UNROLL for (int k = 0; k < 3; ++k) forget(sp[n][k]); }
                                UNROLL for (int j = 0; j < NF; ++j) { forget(y[j]); forget(xa[j]); forget(wc[j]); }
                                UNROLL for (int k = 0; k < 6; ++k) { forget(ry[k]); forget(ra[k]); }
                            }
                        }
                    }
                    i0 = maxit;
                    // (where the loop ends by maxit, the problems still iterating store the last iteration's F_{k+1} and its image from the
                    // register set that iteration wrote -- at the exit itself: asked behind the loop which set that was, both stay live through it)
                    if (!pairs_done && act != 0 && maxit > 0) {
                        for (int i = 0;;) {
                            const int r = iterate_k(xa, ra, xb, rb, i);
                            if (r != kGo) { if (r == kHandOver) i0 = i; break; }
                            if (i + 1 >= maxit) { store_fr(act, xb, rb); break; }
                            const int r1 = iterate_k(xb, rb, xa, ra, i + 1);
                            if (r1 != kGo) { if (r1 == kHandOver) i0 = i + 1; break; }
                            i += 2;
                            if (i >= maxit) { store_fr(act, xa, ra); break; }
                        }
                    }
                    const int n0 = (unsigned)act != 0u ? i0 : c0, n1 = (unsigned)(act >> 32) != 0u ? i0 : c1;
                    {   // what the tested loop and the rest of the phase work on comes back (read whether the tested loop runs or not: a
                        // condition here and the registers stay occupied across the loop above)
                        lds_fence();
                        const double *Hd = header(); const int *Hi = reinterpret_cast<const int *>(Hd + 12);
                        L_f = (R)Hd[10]; it_f = Hi[4]; bt_f = Hi[5];
                        it_f += (int)(lane < LPP ? n0 : n1);
                        if (banded != 0) band_L((double)L_f * 0.5, Llo, Lhi);
                        const R *Cz = consts();
                        UNROLL for (int j = 0; j < NF; ++j) wf[j] = Cz[j];
                        UNROLL for (int k = 0; k < 6; ++k) bpk[k] = Cz[NF + k];
                    }
                }
            } else
            if constexpr (CAN_CERT) { if (cert) i0 = loop(0, std::true_type{}); }
            if (i0 < maxit) {
                if (!XLDS && (i0 & 1)) { UNROLL for (int j = 0; j < NF; ++j) xa[j] = xb[j]; UNROLL for (int k = 0; k < 6; ++k) ra[k] = rb[k]; }
                loop(i0, std::false_type{});
            }
        }

        // =================================================================== X step
        {
            if constexpr (MATES) mate_boundary(2 * it + 2);
            if (PARK) park_f();
            const unsigned ph = opaque_zero();
            const unsigned sl_ = XLDS ? opaque_copy(sl) : sl;
            const Off o = XLDS ? make_off(sl_) : Off{oX, oPI, oF, oK, oP9};
            const unsigned oC = o.K * (unsigned)(E * 4);
            R c[E], r[E][3];
            UNROLL for (int n = 0; n < E; ++n) {
                c[n] = ldz<R>(cnt_u, oC + ph, 4 * n, rvalid);
                UNROLL for (int k = 0; k < 3; ++k) r[n][k] = ldz<R>(cnt_u, oC + ph, 4 * n + 1 + k, rvalid);
            }
            // A_f / b_f entries of this knot from the new forces (centroidal.cpp:86-127)
            R SX = 0, SY = 0, SZ = 0, bf[9];
            // (CLDS: the forces come as fv, the F block read in one batch by the caller -- see "phase prologues")
            auto make_bf = [&](const R (&cc)[E], const R (&rr)[E][3], R (&b)[9], R &sx, R &sy, R &sz, [[maybe_unused]] const R *fv) {
                R b3 = 0, b4 = 0, b5 = 0, b6 = 0, b7 = 0, b8 = 0;
                sx = 0; sy = 0; sz = 0;
                UNROLL for (int n = 0; n < E; ++n) {
                    R fx, fy, fz;
                    if constexpr (CLDS) { fx = fv[3 * n]; fy = fv[3 * n + 1]; fz = fv[3 * n + 2]; }
                    else { fx = rvalid ? Fg[3 * n] : R(0); fy = rvalid ? Fg[3 * n + 1] : R(0); fz = rvalid ? Fg[3 * n + 2] : R(0); }
                    sx += cc[n] * fx * dt; sy += cc[n] * fy * dt; sz += cc[n] * fz * dt;
                    b3 += -cc[n] * fx * dt / m; b4 += -cc[n] * fy * dt / m; b5 += -cc[n] * fz * dt / m;
                    b6 += (cc[n] * fy * rr[n][2] - cc[n] * fz * rr[n][1]) * dt;
                    b7 += (cc[n] * fz * rr[n][0] - cc[n] * fx * rr[n][2]) * dt;
                    b8 += (cc[n] * fx * rr[n][1] - cc[n] * fy * rr[n][0]) * dt;
                }
                b[0] = 0; b[1] = 0; b[2] = 0;
                b[3] = b3; b[4] = b4; b[5] = b5 + R(kGravity) * dt;
                b[6] = b6; b[7] = b7; b[8] = b8;
            };
            [[maybe_unused]] R *rec = nullptr;      // CLDS: this prologue's one address of the lane's record (see "phase prologues")
            [[maybe_unused]] R Fv[CLDS ? NF : 1], Pv[CLDS ? 9 : 1];
            if constexpr (CLDS) {
                rec = record_or_front(kvalid_m);
                lds_block(rec + 18, Fv, rvalid);
                lds_batch(rec + 9, Pv);      // (selected with the sum it enters, below)
            }
            make_bf(c, r, bf, SX, SY, SZ, Fv);
            R bpk[9];
            UNROLL for (int l = 0; l < 9; ++l) {
                if constexpr (CLDS) bpk[l] = rvalid ? (-bf[l] + Pv[l]) : R(0);
                else bpk[l] = rvalid ? (-bf[l] + Pg[l]) : R(0);
            }
            // cost and bounds of this knot
            R qd[9], q[9], lb[NB], ub[NB];
            if (RAW) {
                UNROLL for (int l = 0; l < 9; ++l) {
                    if constexpr (BQ) qd[l] = R(0);      // (unused)
                    else qd[l] = ldz<R>(a.Qx + wave0 * nx, o.X + ph, l, kvalid);
                    q[l] = R(0.5) * ldz<R>(a.qx + wave0 * nx, o.X + ph, l, kvalid);     // q/2
                }
                UNROLL for (int l = 0; l < NB; ++l) {
                    const R lo = (R)at(a.lbx + wave0 * nx, o.X + ph)[l], hi = (R)at(a.ubx + wave0 * nx, o.X + ph)[l];
                    lb[l] = kvalid ? lo : R(-INFINITY);
                    ub[l] = kvalid ? hi : R(INFINITY);
                }
            } else {
                // create_cost_X (biconvex.cpp:57-72)
                UNROLL for (int l = 0; l < 9; ++l) {
                    const double w_run = at(a.W_X + wave0 * a.sW_X, 8u * (sl_ * (unsigned)a.sW_X + 9u * tr) + ph)[l];
                    const double w_ter = at(a.W_X_ter + wave0 * a.sW_X_ter, 8u * sl_ * (unsigned)a.sW_X_ter + ph)[l];
                    const double x_run = at(a.X_nom + wave0 * 9L * H, 8u * 9u * (sl_ * (unsigned)H + tr) + ph)[l];
                    const double x_ter = at(a.X_ter + wave0 * 9, o.P9 + ph)[l];
                    const R w = (R)(rvalid ? w_run : (kvalid ? w_ter : 0.0));
                    const R xr = (R)(rvalid ? x_run : (kvalid ? x_ter : 0.0));
                    qd[l] = w;
                    q[l] = -(xr * w);              // q/2 (create_cost_X: q = -2 W x_ref)
                }
                // create_bound_constraints (biconvex.cpp:27-55): CoM box around the feet
                R csum = 0;
                UNROLL for (int n = 0; n < E; ++n) csum += c[n];
                const bool bounded = rvalid && csum > 0;
                UNROLL for (int k = 0; k < 3; ++k) {
                    R mx = r[0][k], mn = r[0][k];
                    UNROLL for (int n = 1; n < E; ++n) { mx = fmaxR(mx, r[n][k]); mn = fminR(mn, r[n][k]); }
                    const double *bnd = at(a.bounds + wave0 * a.sbounds, 8u * (sl_ * (unsigned)a.sbounds + 6u * tr) + ph);
                    const double b_lo = bnd[k], b_hi = bnd[3 + k];
                    const R blo = (R)(bounded ? b_lo : 0.0);
                    const R bhi = (R)(bounded ? b_hi : 0.0);
                    lb[k] = bounded ? mx + blo : R(-INFINITY);
                    ub[k] = bounded ? mn + bhi : R(INFINITY);
                }
            }
            // x_init rows folded into lane 0's diagonal cost:  rho |X_0 + (P_H - x_init)|^2   (q holds q/2: half-gradient form,
            // see the force step)
            R pi[9];
            [[maybe_unused]] R xi9[CLDS ? 9 : 1];
            if constexpr (CLDS) {      // the segment's header holds the x_init rows' multipliers: one address for all its lanes, read by all, kept by lane 0;
                lds_block(header(), pi, l0);      // x_init likewise, as one batch of loads (as `l0 ? pi - xi : 0` alone: nine masked loads, each waited for)
                UNROLL for (int l = 0; l < 9; ++l) xi9[l] = (R)at(xinit_u, o.P9 + ph)[l];
                keep_here(xi9);
            } else {
            UNROLL for (int l = 0; l < 9; ++l) pi[l] = R(0);
            if (l0) { UNROLL for (int l = 0; l < 9; ++l) pi[l] = PIg[l]; }
            }
            UNROLL for (int l = 0; l < 9; ++l) {
                R xi;
                if constexpr (CLDS) xi = xi9[l]; else xi = (R)at(xinit_u, o.P9 + ph)[l];
                const R bpi = l0 ? (pi[l] - xi) : R(0);
                qd[l] += l0 ? rho : R(0);
                q[l] = fmaR(rho, bpi, q[l]);
            }
            [[maybe_unused]] R Qb[BQ ? 45 : 1];      // BQ: the knot's block, its upper triangle (sym_index), lane 0's with rho on its diagonal
            if constexpr (BQ) {
                if (bq.Qx_blk) {
                    const unsigned oB = 8u * (sl_ * (unsigned)bq.sQx_blk + 81u * tk) + ph;
                    UNROLL for (int r = 0; r < 9; ++r) {
                        UNROLL for (int cc = r; cc < 9; ++cc) Qb[sym_index(9, r, cc)] = ldz<R>(bq.Qx_blk + wave0 * bq.sQx_blk, oB, r * 9 + cc, kvalid);
                    }
                } else {      // this side has its diagonal only: the block with exact zeros beside it
                    UNROLL for (int k = 0; k < 45; ++k) Qb[k] = R(0);
                    UNROLL for (int l = 0; l < 9; ++l) Qb[sym_index(9, l, l)] = ldz<R>(a.Qx + wave0 * nx, o.X + ph, l, kvalid);
                }
                UNROLL for (int l = 0; l < 9; ++l) Qb[sym_index(9, l, l)] += l0 ? rho : R(0);
            }
            // KQ: the weights between knots t and t + 1 (ox) and t - 1 and t (oxp)
            [[maybe_unused]] R ox[KQ ? 9 : 1], oxp[KQ ? 9 : 1];
            [[maybe_unused]] const int xpm = kvalid && t >= 1 ? -1 : 0;
            if constexpr (KQ) {
                if (kq.Qx_off) {
                    const unsigned oB = 8u * (sl_ * (unsigned)kq.sQx_off + 9u * tr) + ph;
                    UNROLL for (int l = 0; l < 9; ++l) ox[l] = ldz<R>(kq.Qx_off + wave0 * kq.sQx_off, oB, l, rvalid);
                } else {
                    UNROLL for (int l = 0; l < 9; ++l) ox[l] = R(0);
                }
                shift_prev(ox, oxp);
                UNROLL for (int l = 0; l < 9; ++l) oxp[l] = keep_if(oxp[l], xpm);
            }
            UNROLL for (int l = 0; l < NB; ++l) {   // quieted once, so the clamp is a bare min/max pair
                lb[l] = __builtin_canonicalize(lb[l]);
                ub[l] = __builtin_canonicalize(ub[l]);
            }
            const int rmask = rvalid ? -1 : 0;      // row-block mask: lanes t >= H own no dynamics rows
            // u = A_f v + bPk on row-block t; vn = v of knot t+1
            [[maybe_unused]] R vnx[KQ ? 9 : 1];      // KQ: what applyA fetched last from knot t + 1
            auto applyA = [&](const R (&v)[9], R (&u)[9]) {
                R vn[9];
                shift_next(v, vn);
                if constexpr (KQ) { UNROLL for (int l = 0; l < 9; ++l) vnx[l] = vn[l]; }
                R w[9];
                UNROLL for (int l = 0; l < 9; ++l) w[l] = v[l] - vn[l];
                UNROLL for (int k = 0; k < 3; ++k) w[k] += dt * vn[3 + k];
                w[6] += SY * v[2] - SZ * v[1];
                w[7] += SZ * v[0] - SX * v[2];
                w[8] += SX * v[1] - SY * v[0];
                UNROLL for (int l = 0; l < 9; ++l) u[l] = keep_if(w[l] + bpk[l], rmask);
            };

            R xa[9], xb[9], y[9], ra[9], rb[9], ry[9];
            if constexpr (CLDS) { lds_block(rec, xa, kvalid); UNROLL for (int l = 0; l < 9; ++l) y[l] = xa[l]; }
            else { UNROLL for (int l = 0; l < 9; ++l) { xa[l] = kvalid ? Xg[l] : R(0); y[l] = xa[l]; } }
            applyA(y, ry);
            UNROLL for (int l = 0; l < 9; ++l) ra[l] = ry[l];
            if constexpr (CLDS) { if (kvalid) { UNROLL for (int l = 0; l < 9; ++l) rec[18 + NF + l] = ry[l]; } }
            else
            if (XLDS && kvalid) { UNROLL for (int l = 0; l < 9; ++l) Rg[l] = ry[l]; }
            const double tol2 = tol * tol;
            if (PARK) load_xloop();
            R invL = R(2) * (R(1) / L_x);
            mask_t banded = 0;      // (see the force step)
            float Llo = 0.0f, Lhi = 0.0f;
            if constexpr (BAND) if (a.exact_step_decisions != 1) {
                bool wneg = false;
                UNROLL for (int l = 0; l < 9; ++l) wneg = wneg || qd[l] < R(0);
                banded = rho >= R(0) && __ballot(wneg) == 0 ? ~mask_t(0) : mask_t(0);
                band_L((double)L_x * 0.5, Llo, Lhi);
            }
            mask_t act = alive;
            auto iterate = [&](const R (&xo_reg)[9], const R (&ro_reg)[9], R (&xn)[9], R (&rn)[9], int i) {
                const R cm = (R)cmtab[i];
                R xo[9], ro[9];
                if (!XLDS) { UNROLL for (int l = 0; l < 9; ++l) { xo[l] = xo_reg[l]; ro[l] = ro_reg[l]; } }
                mask_t done;
                mask_t pend = act;
                for (;;) {
                    [[maybe_unused]] R yp[KQ ? 9 : 1], yn[KQ ? 9 : 1];      // KQ: y of knots t - 1 and t + 1 (per trial, see the force step)
                    if constexpr (KQ) {
                        shift_prev(y, yp);
                        shift_next(y, yn);
                        UNROLL for (int l = 0; l < 9; ++l) { yp[l] = keep_if(yp[l], xpm); yn[l] = keep_if(yn[l], rmask); }
                    }
                    {   // half gradient Q y + q/2 + rho A_f^T (A_f y + bPk), step, box projection (fista.cpp:10); inside the retry
                        // loop like the force step's
                        R z[9], wp[9];
                        shift_prev(ry, wp);  // row-block t-1 (0 for t == 0)
                        UNROLL for (int l = 0; l < 9; ++l) z[l] = ry[l] - wp[l];
                        UNROLL for (int k = 0; k < 3; ++k) z[3 + k] = fmaR(dtp, wp[k], z[3 + k]);
                        z[0] += SZ * ry[7] - SY * ry[8];
                        z[1] += SX * ry[8] - SZ * ry[6];
                        z[2] += SY * ry[6] - SX * ry[7];
                        UNROLL for (int l = 0; l < 9; ++l) {
                            R g = fmaR(rho, z[l], q[l]);
                            if constexpr (BQ) { UNROLL for (int j = 0; j < 9; ++j) g = fmaR(Qb[sym_index(9, l, j)], y[j], g); }      // row l of Q y, column by column
                            else g = fmaR(qd[l], y[l], g);
                            if constexpr (KQ) { g = fmaR(oxp[l], yp[l], g); g = fmaR(ox[l], yn[l], g); }
                            R v = fmaR(-g, invL, y[l]);
                            if (l < NB) v = clamp_box(v, lb[l], ub[l]);
                            xn[l] = v;
                        }
                    }
                    applyA(xn, rn);
                    R g2 = 0, cv = 0, e2 = 0;
                    [[maybe_unused]] R dx[BQ ? 9 : 1];
                    [[maybe_unused]] R cp = 0;      // KQ: the pairs (t, t + 1), 2 off_t d_t d_{t+1}, summed on their own (see the force step)
                    UNROLL for (int l = 0; l < 9; ++l) {
                        const R d = xn[l] - y[l];
                        const R e = rn[l] - ry[l];
                        g2 = fmaR(d, d, g2);
                        if constexpr (BQ) dx[l] = d;
                        else cv = fmaR(qd[l] * d, d, cv);
                        // KQ: d_{t+1} = xn_{t+1} - y_{t+1} from what applyA fetched (the neighbour lane's bits where that lane is the problem's)
                        if constexpr (KQ) cp = fmaR((ox[l] + ox[l]) * d, vnx[l] - yn[l], cp);
                        e2 = fmaR(e, e, e2);
                    }
                    if constexpr (BQ) {      // d'Q d, row by row
                        UNROLL for (int r = 0; r < 9; ++r) {
                            R qdr = Qb[sym_index(9, r, 0)] * dx[0];
                            UNROLL for (int j = 1; j < 9; ++j) qdr = fmaR(Qb[sym_index(9, r, j)], dx[j], qdr);
                            cv = fmaR(qdr, dx[r], cv);
                        }
                    }
                    if constexpr (KQ) cv += keep_if(cp, rmask);
                    cv = fmaR(rho, e2, cv);
                    if (XLDS) { UNROLL for (int l = 0; l < 9; ++l) { xo[l] = Xz[l]; ro[l] = RXz[l]; } }      // (see the force step)
                    mask_t bt;
                    if constexpr (BAND) {
                        mask_t unclear = ~mask_t(0);
                        bt = 0;
                        if (banded != 0) {      // the fp32 decisions, if every live problem's are clear (see the force step)
                            float gf = (float)g2, cf = (float)cv;
                            seg_sum2_f32<LPP>(gf, cf);
                            const mask_t yes = __ballot(cf > gf * Lhi), no = __ballot(cf < gf * Llo);
                            const mask_t dyes = __ballot(gf < t2lo), dno = __ballot(gf > t2hi);
                            const mask_t clear = (yes | no) & (dyes | dno) & __ballot(gf >= 1e-24f) & __ballot(gf <= 1e30f);
                            unclear = ~clear & seg_desig<LPP>() & act;
                            if (unclear == 0) { bt = yes; done = dyes; }
                        }
                        if (unclear != 0) {
                            double g2s = (double)g2, cvs = (double)cv;
                            sum2(g2s, cvs);
                            const double Lh = (double)L_x * 0.5, rhs = Lh * g2s;   // see the force loop for the sqrt-free form
                            bt = __ballot(cvs > rhs);
                            done = __ballot(g2s < tol2);
                            const mask_t edge = __ballot((fabs(cvs - rhs) <= 1e-14 * rhs) || (fabs(g2s - tol2) <= 1e-14 * tol2)) & seg_desig<LPP>();
                            if (edge != 0) {
                                const double Gn = sqrt(g2s);
                                bt = __ballot(cvs > Lh * (Gn * Gn));
                                done = __ballot(Gn < tol);
                            }
                        }
                    } else {
                        double g2s = (double)g2, cvs = (double)cv;
                        sum2(g2s, cvs);
                        const double Lh = (double)L_x * 0.5, rhs = Lh * g2s;   // see the force loop for the sqrt-free form
                        bt = __ballot(cvs > rhs);
                        done = __ballot(g2s < tol2);
                        const mask_t edge = __ballot((fabs(cvs - rhs) <= 1e-14 * rhs) || (fabs(g2s - tol2) <= 1e-14 * tol2)) & seg_desig<LPP>();
                        if (edge != 0) {
                            const double Gn = sqrt(g2s);
                            bt = __ballot(cvs > Lh * (Gn * Gn));
                            done = __ballot(Gn < tol);
                        }
                    }
                    bt = seg_uniform<LPP>(bt);      // (LPP = 21: the sums live at three lanes; their decisions go to their segments)
                    done = seg_uniform<LPP>(done);
                    if (XLDS) { UNROLL for (int l = 0; l < 9; ++l) { keep_here(xo[l]); keep_here(ro[l]); } }
                    bt &= pend;
                    pend = bt;
                    if (bt == 0) break;
                    if (lanes(bt)) { L_x *= beta; ++bt_x; }
                    invL = R(2) * (R(1) / L_x);
                    if constexpr (BAND) if (banded != 0) band_L((double)L_x * 0.5, Llo, Lhi);
                }
                if (!XLDS) {
                    const mask_t last = act & (i == maxit - 1 ? ~mask_t(0) : done) & kvalid_m;
                    if (lanes(last)) { UNROLL for (int l = 0; l < 9; ++l) Xg[l] = xn[l]; }
                }
                UNROLL for (int l = 0; l < 9; ++l) {
                    y[l] = fmaR(cm, xn[l] - xo[l], xn[l]);
                    ry[l] = fmaR(cm, rn[l] - ro[l], rn[l]);
                }
                if (XLDS && lanes(act & kvalid_m)) { UNROLL for (int l = 0; l < 9; ++l) { Xg[l] = xn[l]; Rg[l] = rn[l]; } }
                it_x += lanes(act) ? 1 : 0;
                act &= ~done;
            };
            if constexpr (BAND) {
                // The step certificate of a motion phase (tools/certify_rate.py: motion_bound_terms).  M = Q + rho A_f'A_f
                // couples knot t with t + 1: with dg = diag(M) (lane 0's Q carries the rho of the folded x_init rows), u = |A_f| dg -- row
                // block t takes dg of knots t and t + 1 -- and v = |A_f|' u -- knot t takes u of row blocks t and t - 1 -- the lane's
                // rows pass if Q_i dg_i + rho v_i <= T dg_i.  Two wave shifts of nine values per phase; what a shift brings across the
                // end of a segment is removed by keep_if (a diverged wave-mate's NaNs stay its own), NaN inputs fail the comparison.
                bool cert = false;
                double floor2 = 0.0;
                if (a.certified_steps == 1) {
                    const double Lh0 = (double)L_x * 0.5, T = Lh0 * (1.0 - kCertEta);
                    const double ax = fabs((double)SX), ay = fabs((double)SY), az = fabs((double)SZ);
                    const double cn = (rvalid ? 1.0 : 0.0) + (kvalid && t >= 1 ? 1.0 : 0.0);      // the 1 / -1 of row blocks t and t - 1
                    double dg[9], dgn[9], u[9], up[9], x2 = 0.0, b2 = 0.0;
                    const double col[9] = {cn + (ay * ay + az * az), cn + (ax * ax + az * az), cn + (ax * ax + ay * ay),
                                           cn + (double)dtp * (double)dtp, cn + (double)dtp * (double)dtp, cn + (double)dtp * (double)dtp, cn, cn, cn};
                    UNROLL for (int l = 0; l < 9; ++l) dg[l] = (double)qd[l] + (double)rho * col[l];
                    shift_next(dg, dgn);
                    UNROLL for (int l = 0; l < 9; ++l) { dgn[l] = keep_if(dgn[l], rmask); u[l] = dg[l] + dgn[l]; }
                    UNROLL for (int k = 0; k < 3; ++k) u[k] += (double)dt * dgn[3 + k];
                    u[6] += az * dg[1] + ay * dg[2];
                    u[7] += az * dg[0] + ax * dg[2];
                    u[8] += ay * dg[0] + ax * dg[1];
                    UNROLL for (int l = 0; l < 9; ++l) u[l] = keep_if(u[l], rmask);
                    shift_prev(u, up);
                    UNROLL for (int l = 0; l < 9; ++l) up[l] = keep_if(up[l], xpm);
                    double v[9];
                    UNROLL for (int l = 0; l < 9; ++l) v[l] = u[l] + up[l];
                    UNROLL for (int k = 0; k < 3; ++k) v[3 + k] += (double)dtp * up[k];
                    v[0] += az * u[7] + ay * u[8];
                    v[1] += az * u[6] + ax * u[8];
                    v[2] += ay * u[6] + ax * u[7];
                    bool ok = true;
                    UNROLL for (int l = 0; l < 9; ++l) ok = ok && (double)qd[l] * dg[l] + (double)rho * v[l] <= T * dg[l];
                    if constexpr (CLDS) { UNROLL for (int l = 0; l < 9; ++l) x2 += (double)xa[l] * (double)xa[l]; }      // (x_0, still in xa; a lane without a knot: exact zeros)
                    else
                    if (kvalid) { UNROLL for (int l = 0; l < 9; ++l) x2 += (double)Xg[l] * (double)Xg[l]; }      // (x_0: the X block)
                    UNROLL for (int l = 0; l < 9; ++l) b2 += (double)bpk[l] * (double)bpk[l];
                    cert = certify(ok, alive);
                    if (cert) floor2 = cert_floor(b2 + (T / (double)rho) * x2, Lh0, alive);
                }
                if (cert && l0 && lanes(alive)) ++cert_count()[1];
                float flo = 0.0f, fhi = 0.0f;
                if (banded != 0) band_u(floor2, flo, fhi);
                const double theta = cert && a.exact_step_decisions == 0 ? screen_theta(tol2, floor2) : __builtin_inf();      // (see the force step)
                // one iteration of the certified loop: the tested loop's step, momentum and write-back, operation for operation, without
                // the image difference, cv and the retry loop around them (bt = 0 whatever the step); a live problem's step below the
                // floor commits nothing and hands the phase to the tested loop from this iteration (x_k and its image are in LDS: nothing
                // to move)
                // ... and A_f of the certified loop: applyA without the row mask.  The image of a lane without a dynamics row (t >= H) is
                // not zeroed but never used: its ry is not advanced (it stays the exact zero the phase's first, masked applyA(y, ry) left)
                // and its R block is not written (knot H's keeps those zeros, which the tested loop reads after a hand-over and, through
                // ry, lane 0 of the next segment when H = 31).  What a wave shift brings across a segment's end -- a diverged wave-mate's
                // NaN -- therefore ends in those unused values; the lane a shift reads across the end is always one with t >= H.
                auto applyA_c = [&](const R (&v)[9], R (&u)[9]) {
                    R vn[9];
                    shift_next(v, vn);
                    R w[9];
                    UNROLL for (int l = 0; l < 9; ++l) w[l] = v[l] - vn[l];
                    UNROLL for (int k = 0; k < 3; ++k) w[k] += dt * vn[3 + k];
                    w[6] += SY * v[2] - SZ * v[1];
                    w[7] += SZ * v[0] - SX * v[2];
                    w[8] += SX * v[1] - SY * v[0];
                    UNROLL for (int l = 0; l < 9; ++l) u[l] = w[l] + bpk[l];
                };
                auto iterate_c = [&](int i) -> bool {
                    const R cm = (R)cmtab[i];
                    R xn[9], rn[9], xo[9], ro[9];
                    mask_t done;
                    {
                        R z[9], wp[9];
                        shift_prev(ry, wp);  // row-block t-1 (0 for t == 0)
                        UNROLL for (int l = 0; l < 9; ++l) z[l] = ry[l] - wp[l];
                        UNROLL for (int k = 0; k < 3; ++k) z[3 + k] = fmaR(dtp, wp[k], z[3 + k]);
                        z[0] += SZ * ry[7] - SY * ry[8];
                        z[1] += SX * ry[8] - SZ * ry[6];
                        z[2] += SY * ry[6] - SX * ry[7];
                        UNROLL for (int l = 0; l < 9; ++l) {
                            R g = fmaR(rho, z[l], q[l]);
                            g = fmaR(qd[l], y[l], g);
                            R v = fmaR(-g, invL, y[l]);
                            if (l < NB) v = clamp_box(v, lb[l], ub[l]);
                            xn[l] = v;
                        }
                    }
                    applyA_c(xn, rn);
                    R g2 = 0, s = 0;
                    UNROLL for (int k = 0; k < (int)(sizeof(kScreenTermsX) / sizeof(int)); ++k) { const R d = xn[kScreenTermsX[k]] - y[kScreenTermsX[k]]; s = fmaR(d, d, s); }
                    UNROLL for (int l = 0; l < 9; ++l) { xo[l] = Xz[l]; ro[l] = RXz[l]; }      // (see the force step)
                    bool settled = seg_covered<LPP>(__ballot(s > theta), act);      // the screen, stage 1 (see the force step)
                    if (!settled) {      // stage 2: the whole partial, with the bits it always had
                        UNROLL for (int l = 0; l < 9; ++l) { const R d = xn[l] - y[l]; g2 = fmaR(d, d, g2); }
                        settled = seg_covered<LPP>(__ballot(g2 > theta), act);
                    }
                    if (settled) done = 0;
                    else {
                        mask_t unclear = ~mask_t(0);
                        if (banded != 0) {      // the fp32 decisions -- floor and exit -- if every live problem's are clear (see the force step)
                            float gf = (float)g2;
                            seg_sum1_f32<LPP>(gf);
                            const mask_t yes = __ballot(gf < flo), no = __ballot(gf > fhi);
                            const mask_t dyes = __ballot(gf < t2lo), dno = __ballot(gf > t2hi);
                            const mask_t clear = (yes | no) & (dyes | dno) & __ballot(gf >= 1e-24f) & __ballot(gf <= 1e30f);
                            unclear = ~clear & act;
                            if (unclear == 0) {
                                if ((yes & act) != 0) return false;
                                done = dyes;
                            }
                        }
                        if (unclear != 0) {
                            double g2s = (double)g2;
                            sum1(g2s);
                            if ((__ballot(g2s < floor2) & act) != 0) return false;
                            done = __ballot(g2s < tol2);      // the tested loop's exit rule (see the force loop for the sqrt-free form)
                            if (__ballot(fabs(g2s - tol2) <= 1e-14 * tol2) != 0) done = __ballot(sqrt(g2s) < tol);
                        }
                    }
                    UNROLL for (int l = 0; l < 9; ++l) { keep_here(xo[l]); keep_here(ro[l]); }
                    UNROLL for (int l = 0; l < 9; ++l) y[l] = fma3(cm, xn[l] - xo[l], xn[l]);      // (no copies at the loop's end: see fma3)
                    if (rvalid) { UNROLL for (int l = 0; l < 9; ++l) ry[l] = fmaR(cm, rn[l] - ro[l], rn[l]); }      // (see applyA_c)
                    if (lanes(act & kvalid_m)) { UNROLL for (int l = 0; l < 9; ++l) Xg[l] = xn[l]; }
                    if (lanes(act & rvalid_m)) { UNROLL for (int l = 0; l < 9; ++l) Rg[l] = rn[l]; }
                    it_x += lanes(act) ? 1 : 0;
                    act &= ~done;
                    return true;
                };
                int i0 = 0;
                if constexpr (CLDS) {
                    // CLDS: the certified loop with x_k and its image in REGISTERS (xa / ra and xb / rb, roles alternating as in the tested
                    // loop of the one-wave build) and 18 of the phase's constants -- q and bPk -- in LDS: the knot's record of kLoopConstLds
                    // doubles behind the wave's two problems (lanes without a knot read the zeros, which is what their q and bPk are up to
                    // the sign of a zero that only their own unused values see).  A constant has no producer inside the loop: q comes in
                    // during the previous iteration's momentum step, bPk behind the gradient step (used last in A x+, after the step
                    // decisions), and nothing is written back.  The address passes through opaque_copy in every iteration, or the loads
                    // leave the loop and their values spill.  What the tested loop needs behind this one (q, bPk, L_x, the counters, the
                    // thresholds of L) is read back from LDS, so that it does not occupy registers across the loop.
                    // iterate_c's operations on the same operands in the same order: the same bits.
                    // What the X / R blocks of LDS hold is now written only where it is read again:
                    //   * a problem whose `done` bit rises, or one still iterating at maxit - 1, stores x_{k+1} and its image there (what
                    //     iterate_c leaves under `act` in every iteration: the phase's result, and what a later hand-over finds);
                    //   * a hand-over (a live problem's step below the floor) first stores x_k and its image for the problems still
                    //     iterating, so the tested loop -- in the XLDS form -- finds what iterate_c would have left.
                    // A lane stores its own values to its own record under its own problem's mask, and the R block only where it owns a
                    // dynamics row: knot H's R block and ry keep the exact zeros applyA_c's argument rests on, and what a wave shift brings
                    // across a segment's end still ends in the image of a lane with t >= H, which is neither advanced into ry nor stored.
                    const unsigned cb = consts_offset(kvalid_m);
                    auto consts = [&]() { return reinterpret_cast<R *>(reinterpret_cast<char *>(lds_raw) + opaque_copy(cb)); };
                    if (cert) {
                        if (kvalid) { R *Cg = consts(); UNROLL for (int l = 0; l < 9; ++l) { Cg[l] = q[l]; Cg[9 + l] = bpk[l]; } }
                        lds_fence();
                        R qc[9];
                        { const R *Cz = consts(); UNROLL for (int l = 0; l < 9; ++l) qc[l] = Cz[l]; }
                        // What an iteration that settles at the screen runs beside its arithmetic is kept to a few scalar instructions:
                        //   * a problem's iteration count is the index at which its bit left `act` (plus one), or the index at which the
                        //     loop ended -- `act` only loses bits here -- noted where `done` has a bit and behind the loop;
                        //   * `act`, the latch of a finishing problem and the words of the screen change only where `done` has a bit;
                        //   * x_{k+1} and its image of the problems still iterating when the loop ends by maxit are stored at that exit of
                        //     the loop, from the register set the copy in front of it wrote;
                        //   * the momentum coefficient is a scalar, loaded one iteration ahead (uniform_load);
                        //   * iterate_k says how the loop goes on by its return value alone: kGo, kHandOver (a live problem's step below
                        //     the floor: nothing of this iteration is kept, the tested loop runs it again) or kAllLeft.
                        int c0 = 0, c1 = 0;      // iterations of the wave's two problems that have left the loop (scalar registers)
                        unsigned dead0, dead1;
                        seg_dead32(act, dead0, dead1);
                        R cmn = uniform_load(cmtab, 0u);
                        auto store_xr = [&](mask_t m, const R (&xv)[9], const R (&rv)[9]) {
                            R *Xs = knot_record();
                            if (lanes(m & kvalid_m)) { UNROLL for (int l = 0; l < 9; ++l) Xs[l] = xv[l]; }
                            if (lanes(m & rvalid_m)) { UNROLL for (int l = 0; l < 9; ++l) Xs[18 + NF + l] = rv[l]; }
                        };
                        auto hand_over = [&](const R (&xo)[9], const R (&ro)[9]) { store_xr(act, xo, ro); };
                        constexpr int kGo = 0, kHandOver = 1, kAllLeft = 2;
                        // an iteration that the screen does not settle: the step decisions from the sums, a hand-over, or problems that finish
                        auto unsettled = [&](const R (&xo)[9], const R (&ro)[9], const R (&xn)[9], const R (&rn)[9], int i, R g2) -> int {
                            mask_t done = 0;
                            mask_t unclear = ~mask_t(0);
                            if (banded != 0) {      // the fp32 decisions -- floor and exit -- if every live problem's are clear (see the force step)
                                float gf = (float)g2;
                                seg_sum1_f32<LPP>(gf);
                                const mask_t yes = __ballot(gf < flo), no = __ballot(gf > fhi);
                                const mask_t dyes = __ballot(gf < t2lo), dno = __ballot(gf > t2hi);
                                const mask_t clear = (yes | no) & (dyes | dno) & __ballot(gf >= 1e-24f) & __ballot(gf <= 1e30f);
                                unclear = ~clear & act;
                                if (unclear == 0) {
                                    if ((yes & act) != 0) { hand_over(xo, ro); return kHandOver; }
                                    done = dyes;
                                }
                            }
                            if (unclear != 0) {
                                double g2s = (double)g2;
                                sum1(g2s);
                                if ((__ballot(g2s < floor2) & act) != 0) { hand_over(xo, ro); return kHandOver; }
                                done = __ballot(g2s < tol2);      // the tested loop's exit rule (see the force loop for the sqrt-free form)
                                if (__ballot(fabs(g2s - tol2) <= 1e-14 * tol2) != 0) done = __ballot(sqrt(g2s) < tol);
                            }
                            const mask_t latch = act & done;
                            if (latch != 0) {      // problems that finish here: x_{k+1} and its image, their counts, and what follows from `act`
                                store_xr(latch, xn, rn);
                                if ((unsigned)latch != 0u) c0 = i + 1;
                                if ((unsigned)(latch >> 32) != 0u) c1 = i + 1;
                                act &= ~done;
                                if (act == 0) return kAllLeft;      // (nothing reads y behind the loop)
                                seg_dead32(act, dead0, dead1);
                            }
                            return kGo;
                        };
                        auto iterate_k = [&](const R (&xo)[9], const R (&ro)[9], R (&xn)[9], R (&rn)[9], int i) -> int {
                            const R cm = cmn;
                            cmn = uniform_load(cmtab, min((unsigned)i + 1u, (unsigned)kMaxFistaIters - 1u));      // (the next iteration's)
                            {
                                R z[9], wp[9];
                                shift_prev(ry, wp);  // row-block t-1 (0 for t == 0)
                                UNROLL for (int l = 0; l < 9; ++l) z[l] = ry[l] - wp[l];
                                UNROLL for (int k = 0; k < 3; ++k) z[3 + k] = fmaR(dtp, wp[k], z[3 + k]);
                                z[0] += SZ * ry[7] - SY * ry[8];
                                z[1] += SX * ry[8] - SZ * ry[6];
                                z[2] += SY * ry[6] - SX * ry[7];
                                UNROLL for (int l = 0; l < 9; ++l) {
                                    R g = fmaR(rho, z[l], qc[l]);
                                    g = fmaR(qd[l], y[l], g);
                                    R v = fmaR(-g, invL, y[l]);
                                    if (l < NB) v = clamp_box(v, lb[l], ub[l]);
                                    xn[l] = v;
                                }
                            }
                            {   // applyA_c, its bPk read behind the gradient step (z and its neighbour's image are dead by then) and used last,
                                // behind one wait for all nine
                                R bk[9];
                                const R *Cz = reinterpret_cast<const R *>(reinterpret_cast<const char *>(lds_raw) + opaque_copy_after(cb, xn[8]));
                                UNROLL for (int l = 0; l < 9; ++l) bk[l] = Cz[9 + l];
                                R vn[9], w[9];
                                shift_next(xn, vn);
                                UNROLL for (int l = 0; l < 9; ++l) w[l] = xn[l] - vn[l];
                                UNROLL for (int k = 0; k < 3; ++k) w[k] += dt * vn[3 + k];
                                w[6] += SY * xn[2] - SZ * xn[1];
                                w[7] += SZ * xn[0] - SX * xn[2];
                                w[8] += SX * xn[1] - SY * xn[0];
                                keep_here(bk);
                                UNROLL for (int l = 0; l < 9; ++l) rn[l] = w[l] + bk[l];
                            }
                            R s = 0;
                            UNROLL for (int k = 0; k < (int)(sizeof(kScreenTermsX) / sizeof(int)); ++k) { const R d = xn[kScreenTermsX[k]] - y[kScreenTermsX[k]]; s = fmaR(d, d, s); }
                            // the screen (see the force step); its two stages and what follows a miss are nested branches: as a bool
                            // that the stages share, `settled` is made a 64-bit mask and tested again
                            if (!seg_covered32(__ballot(s > theta), dead0, dead1)) {
                                R g2 = 0;      // stage 2: the whole partial, with the bits it always had
                                UNROLL for (int l = 0; l < 9; ++l) { const R d = xn[l] - y[l]; g2 = fmaR(d, d, g2); }
                                const mask_t own = __ballot(g2 > theta);
                                if (!seg_covered32(own, dead0, dead1) && !seg_covered32(own | quad_screen(g2, theta), dead0, dead1)) {      // stage 3: the lane's quad (biconvex_lanes.h)
                                    const int r = unsettled(xo, ro, xn, rn, i, g2);
                                    if (r != kGo) return r;
                                }
                            }
                            { const R *Cz = consts(); UNROLL for (int l = 0; l < 9; ++l) qc[l] = Cz[l]; }      // (the next iteration's)
                            UNROLL for (int l = 0; l < 9; ++l) y[l] = fma3_s(cm, xn[l] - xo[l], xn[l]);      // (no copies at the loop's end: see fma3)
                            if (rvalid) { UNROLL for (int l = 0; l < 9; ++l) ry[l] = fmaR(cm, rn[l] - ro[l], rn[l]); }      // (see applyA_c)
                            keep_here(qc);      // (a use that stays here: the loads are not sunk to the gradient step; one statement, one wait)
                            return kGo;
                        };
                        i0 = maxit;
                        // (where the loop ends by maxit, the problems still iterating store the last iteration's x_{k+1} and its image from the
                        // register set that iteration wrote -- at the exit itself: asked behind the loop which set that was, both stay live through it)
                        if (act != 0 && maxit > 0) {
                            for (int i = 0;;) {
                                const int r = iterate_k(xa, ra, xb, rb, i);
                                if (r != kGo) { if (r == kHandOver) i0 = i; break; }
                                if (i + 1 >= maxit) { store_xr(act, xb, rb); break; }
                                const int r1 = iterate_k(xb, rb, xa, ra, i + 1);
                                if (r1 != kGo) { if (r1 == kHandOver) i0 = i + 1; break; }
                                i += 2;
                                if (i >= maxit) { store_xr(act, xa, ra); break; }
                            }
                        }
                        const int n0 = (unsigned)act != 0u ? i0 : c0, n1 = (unsigned)(act >> 32) != 0u ? i0 : c1;
                        // (the step constant and the counters are read again from the header, where they have not changed: not held across the loop)
                        load_xloop();
                        if (banded != 0) band_L((double)L_x * 0.5, Llo, Lhi);
                        it_x += (int)(lane < LPP ? n0 : n1);
                        {   // the tested loop takes q and bPk from where the certified one had them (read whether it runs or not: a
                            // condition here and their registers stay occupied across the loop above)
                            lds_fence();
                            const R *Cz = consts();
                            UNROLL for (int l = 0; l < 9; ++l) { q[l] = Cz[l]; bpk[l] = Cz[9 + l]; }
                        }
                    }
                } else
                if (cert) {
                    for (; i0 < maxit; ++i0) {
                        if (act == 0) break;
                        if (!iterate_c(i0)) break;
                    }
                }
                // the tested loop, from the iteration the certified one left undone
                for (int i = i0; i < maxit; i += 2) {
                    if (act == 0) break;
                    iterate(xa, ra, xb, rb, i);
                    if (i + 1 >= maxit || act == 0) break;
                    iterate(xb, rb, xa, ra, i + 1);
                }
            } else {
            for (int i = 0; i < maxit; i += 2) {
                if (act == 0) break;
                iterate(xa, ra, xb, rb, i);
                if (i + 1 >= maxit || act == 0) break;
                iterate(xb, rb, xa, ra, i + 1);
            }
            }
            R fin[9];
            [[maybe_unused]] R *rec2 = nullptr;      // CLDS: the record's address again, for what follows the loops (not held across them)
            [[maybe_unused]] R Fv2[CLDS ? NF : 1];
            if constexpr (CLDS) {
                rec2 = record_or_front(kvalid_m);
                lds_block(rec2, fin, kvalid);
                lds_block(rec2 + 18, Fv2, rvalid);
            } else {
            UNROLL for (int l = 0; l < 9; ++l) fin[l] = kvalid ? Xg[l] : R(0);
            }
            if (PARK) load_rest();
            if (XLDS) {     // b_f made again from the contact plan and the forces (same expressions, same bits) instead of six registers held
                            // across the FISTA loop -- which the 256-register build held in scratch memory
                const unsigned ph2 = opaque_zero();
                R c2[E], r2[E][3], s0, s1, s2;
                UNROLL for (int n = 0; n < E; ++n) {
                    c2[n] = ldz<R>(cnt_u, oC + ph2, 4 * n, rvalid);
                    UNROLL for (int k = 0; k < 3; ++k) r2[n][k] = ldz<R>(cnt_u, oC + ph2, 4 * n + 1 + k, rvalid);
                }
                make_bf(c2, r2, bf, s0, s1, s2, Fv2);
            }

            // dyn_violation = A_f X - b_f ; P += dyn_violation          (biconvex.cpp:98-99)
            double v2 = 0;   // the dynamics violation is accumulated in fp64 whatever R is
            {
                R xn[9], w[9];
                shift_next(fin, xn);
                UNROLL for (int l = 0; l < 9; ++l) w[l] = fin[l] - xn[l];
                UNROLL for (int k = 0; k < 3; ++k) w[k] += dt * xn[3 + k];
                w[6] += SY * fin[2] - SZ * fin[1];
                w[7] += SZ * fin[0] - SX * fin[2];
                w[8] += SX * fin[1] - SY * fin[0];
                const bool al = lanes(alive);
                R dr[9], dx0[9];
                [[maybe_unused]] R xi9[CLDS ? 9 : 1];
                if constexpr (CLDS) {      // (x_init as one batch of loads: see the prologue)
                    const unsigned ph3 = opaque_zero();
                    UNROLL for (int l = 0; l < 9; ++l) xi9[l] = (R)at(xinit_u, o.P9 + ph3)[l];
                    keep_here(xi9);
                }
                UNROLL for (int l = 0; l < 9; ++l) {
                    const R d = rvalid ? (w[l] - bf[l]) : R(0);
                    R xi;
                    if constexpr (CLDS) xi = xi9[l]; else xi = (R)at(xinit_u, o.P9 + ph)[l];
                    const R di = l0 ? (fin[l] - xi) : R(0);
                    dr[l] = d; dx0[l] = di;
                    // (CLDS: the sum as every build has compiled it, spelled out -- d d + (di di) with the first product fused; left to the
                    // compiler's contraction, the straight-line form of this block fused the other product: 1 ulp in dyn_viol)
                    if constexpr (CLDS) v2 += __builtin_fma((double)d, (double)d, (double)di * (double)di);
                    else
                    v2 += (double)d * (double)d + (double)di * (double)di;
                }
                if constexpr (CLDS) {      // (the multipliers' read-modify-write stays under its masks, one region per block)
                    if (al && rvalid) { UNROLL for (int l = 0; l < 9; ++l) rec2[9 + l] += dr[l]; }
                    if (al && l0) { double *Hs = header(); UNROLL for (int l = 0; l < 9; ++l) Hs[l] += dx0[l]; }
                } else {
                if (al && rvalid) { UNROLL for (int l = 0; l < 9; ++l) Pg[l] += dr[l]; }
                if (al && l0) { UNROLL for (int l = 0; l < 9; ++l) PIg[l] += dx0[l]; }
                }
            }
            if (MW) { double z2 = 0.0; sum2(v2, z2); } else v2 = seg_sum<LPP>(v2);
            const double nrm = sqrt(v2);
            if (lanes(alive)) {
                last_viol = nrm;
                const unsigned row = STEAL ? (unsigned)n_admm : (unsigned)it;      // the ADMM iteration this was, counted per problem
                ++n_admm;
                if (a.hist && l0) *at(a.hist + wave0 * a.c.num_iters, 8u * (sl_ * (unsigned)a.c.num_iters + row)) = nrm;
#ifndef BMPC_NO_TRACE
                if (a.trace && l0) {
                    int *tr = a.trace + ((wave0 + sl_) * a.c.num_iters + row) * 4;
                    tr[0] = it_f; tr[1] = it_x; tr[2] = bt_f; tr[3] = bt_x;
                }
#endif
                if (isnan(nrm)) status = 2;                                   // biconvex.cpp:106-109
            }
            const mask_t ex = __ballot(isnan(nrm) || nrm < exit_tol);         // biconvex.cpp:106-109, 111-114
            if (!STEAL) alive &= ~ex;
            else {
                // segments whose problem is over (exit, NaN, or all its iterations run): results out, the next problem in
                const mask_t fin = alive & (ex | __ballot(n_admm >= a.c.num_iters));
                if (fin != 0) {
                    store_problem(fin);
                    int np = -1;
                    if (lanes(fin) && l0) np = (int)((long)gridDim.x * (64 / LPP)) + atomicAdd(a.queue, 1);
                    static_assert(!STEAL || LPP == 21, "the segment broadcast below is written for three segments of 21 lanes");
                    const int n0 = __builtin_amdgcn_readlane(np, 0), n1 = __builtin_amdgcn_readlane(np, 21), n2 = __builtin_amdgcn_readlane(np, 42);
                    const int mine = seg == 0 ? n0 : (seg == 1 ? n1 : n2);
                    const mask_t got = fin & __ballot(pvalid && mine >= 0 && mine < a.B);
                    if (lanes(got)) { prob = mine; sl = (unsigned)mine; set_offsets(); }
                    const R ndt = ldz<R>(a.dt, oK, 0, rvalid);
                    if (lanes(got)) dt = ndt;
                    dtp = from_prev(dt);
                    load_problem(got);
                    alive = (alive & ~fin) | got;
                }
            }
        }
    }
    if constexpr (MATES) mate_boundary(kMateDone);      // (the solve is over: the mate keeps no priority against a wave that only stores its results)
    if constexpr (CLDS) {     // ---- results, with the record's address and the offsets made here (held from the kernel's start they are registers -- or scratch reloads -- of every phase)
        const R *re = record_or_front(kvalid_m);
        const double *He = header();
        const unsigned sle = opaque_copy(sl);
        const Off oe = make_off(sle);
        if (kvalid) { UNROLL for (int l = 0; l < 9; ++l) at(Xu, oe.X)[l] = (double)re[l]; }
        if (rvalid) {
            UNROLL for (int j = 0; j < NF; ++j) at(Fu, oe.F)[j] = (double)re[18 + j];
            UNROLL for (int l = 0; l < 9; ++l) at(Pu, oe.X)[l] = (double)re[9 + l];
        }
        if (l0) { UNROLL for (int l = 0; l < 9; ++l) at(Pu, oe.PI)[l] = (double)He[l]; }
        if (l0) {
            *at(a.L_x + wave0, 8u * sle) = (double)L_x;
            *at(a.L_f + wave0, 8u * sle) = (double)L_f;
            if (a.dyn_viol) *at(a.dyn_viol + wave0, 8u * sle) = last_viol;
            if (a.stats) {
                int *s = a.stats + (wave0 + sle) * kStats;
                s[0] = n_admm; s[1] = it_f; s[2] = it_x; s[3] = bt_f; s[4] = bt_x; s[5] = status;
            }
            if (a.cert_phases) { int *o = a.cert_phases + (wave0 + sle) * 2; const int *cn = cert_count(); o[0] = cn[0]; o[1] = cn[1]; }
        }
#ifdef BMPC_SIMD_STAMPS
        simd_stamp(a.simd_stamps, false);
#endif
    } else
    if (!STEAL) {     // ---- results: one pass from LDS to the output blocks
        if (kvalid) { UNROLL for (int l = 0; l < 9; ++l) at(Xu, oX)[l] = (double)Xg[l]; }
        if (rvalid) {
            UNROLL for (int j = 0; j < NF; ++j) at(Fu, oF)[j] = (double)Fg[j];
            UNROLL for (int l = 0; l < 9; ++l) at(Pu, oX)[l] = (double)Pg[l];
        }
        if (l0) { UNROLL for (int l = 0; l < 9; ++l) at(Pu, oPI)[l] = (double)PIg[l]; }
        if (l0) {
            *at(a.L_x + wave0, 8u * sl) = (double)L_x;
            *at(a.L_f + wave0, 8u * sl) = (double)L_f;
            if (a.dyn_viol) *at(a.dyn_viol + wave0, 8u * sl) = last_viol;
            if (a.stats) {
                int *s = a.stats + (wave0 + sl) * kStats;
                s[0] = n_admm; s[1] = it_f; s[2] = it_x; s[3] = bt_f; s[4] = bt_x; s[5] = status;
            }
            if constexpr (BAND) { if (a.cert_phases) { int *o = a.cert_phases + (wave0 + sl) * 2; o[0] = certn[0]; o[1] = certn[1]; } }
        }
    }
}
