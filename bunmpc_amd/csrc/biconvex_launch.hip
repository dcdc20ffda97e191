// The host launch layer of the batched centroidal ADMM: what a process keeps per device, the dispatch switches, which kernel a batch
// gets (plan_launch) and the launch itself -- and two small kernels beside the solve's own: the lane-exchange self test and the fill
// of FISTA's momentum table.  The solve's kernels are in the units compiled from biconvex_admm.hip (the mapping is described there);
// this file reaches them through the table below and is built with the fp64 units' flags (bunmpc_amd/build.py).
#include "biconvex_kernels.h"
#include <algorithm>
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"

__global__ __launch_bounds__(64) void lane_selftest_kernel(const double *in, double *out) {
    const int i = threadIdx.x;
    const double v = in[i];
    out[i] = from_prev(v);
    out[64 + i] = from_next(v);
    out[128 + i] = seg_sum<16>(v);
    out[192 + i] = seg_sum<32>(v);
    out[256 + i] = seg_sum<64>(v);
    out[320 + i] = (double)__popcll(__ballot(v > 0.0));
    out[384 + i] = seg_sum<21>(i < 63 ? v : 0.0);                                                    // every lane of a 21-lane segment
    double a = i < 63 ? v : 0.0, b = i < 63 ? 2.0 * v : 0.0;
    seg_sum2<21>(a, b);                                                                                // the designated lanes only
    out[448 + i] = a;
    out[512 + i] = b;
    out[576 + i] = (double)seg_uniform<21>(__ballot(v > 40.0) & seg_desig<21>());                  // the spread masks, as a number (< 2^63: exact up to 2^53 -- compared by bits on the host through two halves)
    out[640 + i] = (double)(unsigned)(seg_uniform<21>(__ballot(i == 16 || i == 48)) >> 32);
    out[704 + i] = (double)(unsigned)(seg_uniform<21>(__ballot(i == 16 || i == 48)) & 0xffffffffu);
}

// FISTA's momentum coefficients: t+ = 1 + sqrt(1 + 4 t^2)/2 (sic, fista.cpp:34), c_k = (t_k - 1)/t_{k+1} -- a function of k alone, so
// one table per device, filled once by this kernel (until round 4 every wave tabulated them in its LDS: 1.2 KB of the 20 KB a wave
// may hold when eight of them share a CU)
__global__ void momentum_table_kernel(double *tab, int n) {
    double tk = 1.0;
    for (int i = 0; i < n; ++i) {
        const double tk1 = 1.0 + sqrt(1.0 + 4.0 * tk * tk) * 0.5;
        tab[i] = (tk - 1.0) / tk1;
        tk = tk1;
    }
}
// What a process keeps per device: the momentum table, the work-stealing launches' counters and the chip's size.  (The raised LDS limit
// of a workgroup kernel is per device too: launch_inst, biconvex_admm_inst.h.)
struct DeviceState {
    double *momentum = nullptr;
    int *steal_ring = nullptr;       // 64 counters, one per launch in flight (a launch zeroes its own on its stream in front of the kernel;
    unsigned steal_next = 0;         // with 64 a counter comes round again only after 63 later launches on this device)
    long simds = 0;
};
std::mutex g_device_lock;
// ... of the current device; call with g_device_lock held.  nullptr on error or beyond 16 devices.
DeviceState *device_state() {
    static DeviceState state[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    return &state[dev];
}
long device_simds() {
    std::lock_guard<std::mutex> hold(g_device_lock);
    DeviceState *d = device_state();
    if (d && d->simds) return d->simds;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    if (d) d->simds = 4 * cus;
    return 4 * cus;
}
const double *momentum_table(hipStream_t stream) {
    std::lock_guard<std::mutex> hold(g_device_lock);
    DeviceState *d = device_state();
    if (!d) return nullptr;
    if (!d->momentum) {
        double *t = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&t), kMaxFistaIters * sizeof(double)) != hipSuccess) return nullptr;
        hipLaunchKernelGGL(momentum_table_kernel, dim3(1), dim3(1), 0, stream, t, kMaxFistaIters);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) { (void)hipFree(t); return nullptr; }      // (once per device: later launches on any stream find it filled)
        d->momentum = t;
    }
    return d->momentum;
}
int *steal_counter(hipStream_t stream) {
    std::lock_guard<std::mutex> hold(g_device_lock);
    DeviceState *d = device_state();
    if (!d) return nullptr;
    if (!d->steal_ring && hipMalloc(reinterpret_cast<void **>(&d->steal_ring), 64 * sizeof(int)) != hipSuccess) { d->steal_ring = nullptr; return nullptr; }
    int *c = d->steal_ring + (d->steal_next++ % 64);
    if (hipMemsetAsync(c, 0, sizeof(int), stream) != hipSuccess) return nullptr;
    return c;
}

DispatchKnobs g_knobs;
// of the calling host thread's latest launch_biconvex_admm (tests of the default dispatch; profiles)
thread_local const char *t_last_kernel = "";
thread_local int t_last_lpp = 0, t_last_wpe = 1, t_last_block = 0;

int set_knob(int &knob, int value) { const int old = knob; knob = value; return old; }
#ifdef BMPC_SIMD_STAMPS
// the diagnostic build's stamp buffer (bmpc_simd_stamps_buffer, at the end of this file): the caller's device array, or null
unsigned long long *g_simd_stamps = nullptr;
#endif

// Horizons of 17..21 knots: 32-lane segments (two problems per wave) or 21-lane segments (three per wave), whichever
// finishes the batch sooner.  The kernel runs one wave per SIMD; a wave of three problems takes ~8 % longer than a wave of two
// (the segment sums cost more), so three per wave wins whenever it needs fewer ROUNDS of waves over the chip's SIMDs -- at
// B = 4096 on an MI355X (1024 SIMDs) both need two rounds, 1366 waves or 2048, and two per wave is the faster one; at B = 3072 or
// 6144 three per wave saves a whole round (1.41e6 solves/s against 1.03e6) -- or when the waves' run times differ widely anyway
// (num_iters well above ten: the ADMM's early exit, biconvex.cpp:111-114, makes the iteration counts differ per problem and the
// scheduler backfills; measured at num_iters = 100, B = 4096: 31 -> 28 ms).  (Tried and dropped: B = 4096 as one round of three per
// wave for 3072 problems + the one-problem-per-wave kernel for the other 1024 -- 2.29 + 1.7 ms, level with 2 x 2.02 ms.)
bool three_per_wave_pays(const BatchArgs &a, long simds, const DispatchKnobs &kn) {
    if (kn.three_per_wave != 2) return kn.three_per_wave != 0;
    const long w3 = (a.B + 2) / 3, w2 = (a.B + 1) / 2;
    return (w3 + simds - 1) / simds < (w2 + simds - 1) / simds || a.c.num_iters >= 25;
}
// Two waves per SIMD (the XLDS build) where it is the faster one: the batch needs more waves than the chip has SIMDs.  Results do not
// depend on it.
bool two_per_simd_pays(const BatchArgs &a, int per_wave, long simds, const DispatchKnobs &kn) {
    if (a.precision != 0 || kn.two_per_simd == 0) return false;
    if (kn.two_per_simd == 1) return true;
    return (a.B + per_wave - 1) / per_wave > simds;
}

// The loop-constants build (biconvex_admm_body.h: CLDS) in place of the two-waves build of the 32-lane kernel: four feet, harness
// form, fp64, diagonal costs (the one instantiation it exists in), and a wave's LDS with the constants' area such that eight waves
// still share a CU (loop_constants_fit: 17 .. 21 knots).  Mode 2, "when it pays": see kLoopConstantsPay.  Results do not depend on it.
bool loop_constants_pay(const BatchArgs &a, int n_eff, const DispatchKnobs &kn) {
    if (kn.loop_constants_in_lds == 0 || (kn.loop_constants_in_lds != 1 && !kLoopConstantsPay)) return false;
    return n_eff == 4 && !a.raw && a.precision == 0 && loop_constants_fit(n_eff, a.H);
}

// The loop-constants build in workgroups of eight waves whose SIMD-mates keep level (biconvex_admm_body.h: MATES).  Mode 1 (and 3, the
// geometry without the rule): wherever that build is taken.  Mode 2, "when it pays": where the batch fills the chip exactly once at
// two waves per SIMD -- as many workgroups of 16 problems as the device has CUs (an MI355X: 4081 <= B <= 4096); fewer would leave whole
// CUs empty where one-wave workgroups spread over all of them, more would each wait for a whole CU to drain -- and kSimdMatesPay says
// so.  Results do not depend on it.
bool simd_mates_pay(const BatchArgs &a, long simds, const DispatchKnobs &kn) {
    if (kn.simd_mate_balance == 0 || simd_mates_lds_bytes(4, a.H) > 160 * 1024) return false;
    if (kn.simd_mate_balance == 1 || kn.simd_mate_balance == 3) return true;
    return kSimdMatesPay && ((long)a.B + 15) / 16 == simds / 4;
}

// The units' accessors at 4 * shape + 2 * precision + (two feet), null where kShapes[shape] builds no unit.  Made from kShapes alone: a
// row without its units (bunmpc_amd/build.py lists them) is an undefined symbol when the library loads.
using UnitAccessor = const AdmmUnit &(*)();
struct UnitTable {
    UnitAccessor of[4 * kNumShapes];
};
template <int I>
constexpr UnitAccessor unit_entry() {
    constexpr CostShape SHAPE = (CostShape)(I / 4);
    constexpr int PRECISION = I / 2 % 2, E = I % 2 ? 2 : 4;
    if constexpr (unit_is_built(SHAPE, PRECISION, E)) return &admm_unit_of<SHAPE, PRECISION, E>;
    else return nullptr;
}
template <int... I>
constexpr UnitTable unit_table(std::integer_sequence<int, I...>) { return {{unit_entry<I>()...}}; }
constexpr UnitTable kUnits = unit_table(std::make_integer_sequence<int, 4 * kNumShapes>{});

}  // namespace

const AdmmUnit &admm_unit(CostShape shape, int precision, int n_eff) { return kUnits.of[4 * shape + 2 * precision + (n_eff == 2)](); }

int set_steal_grid(int waves) { return set_knob(g_knobs.steal_grid, waves); }
int set_three_per_wave(int on) { return set_knob(g_knobs.three_per_wave, on); }
int set_two_waves_per_simd(int mode) { return set_knob(g_knobs.two_per_simd, mode); }
int set_work_stealing(int on) { return set_knob(g_knobs.work_stealing, on); }
int set_latency_mapping_max_batch(int max_batch) { return set_knob(g_knobs.latency_max_batch, max_batch); }
int set_exact_step_decisions(int on) { return set_knob(g_knobs.exact_step_decisions, on); }
int set_certified_steps(int on) { return set_knob(g_knobs.certified_steps, on); }
int set_loop_constants_in_lds(int mode) { return set_knob(g_knobs.loop_constants_in_lds, mode); }
int set_force_foot_pairs(int mode) { return set_knob(g_knobs.force_foot_pairs, mode); }
int set_simd_mate_balance(int mode) { return set_knob(g_knobs.simd_mate_balance, mode); }
int biconvex_last_block_size() { return t_last_block; }
int biconvex_last_waves_per_simd() { return t_last_wpe; }
int biconvex_last_lanes_per_problem() { return t_last_lpp; }
const char *biconvex_last_kernel_name() { return t_last_kernel; }

// Which kernel a batch gets.  Block and band costs: their own kernels at every batch size and num_iters -- never the
// one-problem-per-wave, work-stealing, workgroup or two-waves kernels, which hold diagonal weights only -- with every step tested on
// the fp64 sums; the lanes per problem are chosen as for diagonal costs.  The Euclidean cone projection (kCone): likewise, in either form
// (those other kernels restate the reference's projection only); about per-contact normals (kConeFrame): exactly as kCone.
LaunchPlan plan_launch(const BatchArgs &a, CostShape shape, int n_eff, long simds, const DispatchKnobs &kn) {
    LaunchPlan p = {hipErrorInvalidValue, nullptr, {0, false, false, 0, {}, false}, false, a.certified_steps};
    if (shape < 0 || shape >= kNumShapes) return p;
    const ShapeInfo &s = kShapes[shape];
    const bool diag = shape == kDiag;
    const int k = a.H + 1;
    const bool built = k <= s.max_knots && (a.precision == 0 || (a.precision == 1 && !s.fp64_only)) && (a.raw || !s.raw_only);
    if ((n_eff != 2 && n_eff != 4) || a.H < 1 || a.B < 0 || !built) return p;
    if (a.B == 0) { p.status = hipSuccess; return p; }
    if (a.c.maxit > kMaxFistaIters) return p;
    // the kernels address a wave's problems by 32-bit byte offsets from the wave's first problem (at most four problems)
    if (diag || !a.raw)
        for (long stride : {a.sW_X, a.sW_X_ter, a.sW_F, a.sbounds})
            if (stride < 0 || stride > (1L << 26)) return p;
    p.status = hipSuccess;
    // few problems, short horizon: one problem per wave (the chain of a solve is ~2.3x shorter; biconvex_latency.hip)
    if (diag && a.B <= kn.latency_max_batch && latency_mapping_fits(a, n_eff)) {
        p.kernel = "biconvex_latency_kernel";
        p.latency = true;
        return p;
    }
    p.certified_steps = !s.certifies ? 0 : (kn.certified_steps == 2 ? 2 : (kn.certified_steps != 0 ? 1 : 0));      // (2: force phases only)
    p.kernel = diag && a.precision == 1 ? "biconvex_admm_kernel_f32" : s.kernel;
    // the same decisions for two feet as for four, with the LDS record of the foot count (knot_lds)
    auto segments = [&](int lpp) {
        p.l.lpp = lpp;
        p.l.w2 = diag && two_per_simd_pays(a, 64 / lpp, simds, kn);
        p.l.clds = p.l.w2 && lpp == 32 && loop_constants_pay(a, n_eff, kn);
        p.l.mates = p.l.clds && simd_mates_pay(a, simds, kn);
        p.l.mate_rule = p.l.mates && kn.simd_mate_balance != 3 && kSimdMatesRule;
        return p;
    };
    if (k <= 16) return segments(16);
    // 17..21 knots (the headline shape): three problems per wave in 21-lane segments (fp64; the fp32 kernels keep 32-lane segments)
    if (k <= 21 && a.precision == 0 && three_per_wave_pays(a, simds, kn)) {
        // many ADMM iterations (the early exit makes the counts differ per problem) and more waves than the chip holds: segments that
        // finish take the next problem (biconvex_admm_body.h: STEAL); the 32-bit offsets from the problem index must fit (the contact
        // plan: 32 E H bytes per problem)
        const long per = std::max<long>({32L * n_eff * a.H, 9L * (a.H + 1) * 8, a.sW_X * 8, a.sW_F * 8, a.sbounds * 8, (long)a.c.num_iters * 16});
        if (diag && kn.work_stealing && !a.raw && a.c.num_iters >= 25 && (a.B + 2) / 3 > simds && (double)a.B * (double)per < 2.0e9) {
            p.kernel = "biconvex_admm_steal_kernel";
            // (one wave per SIMD unless forced: measured at B = 4096, num_iters = 100: 30.7 ms; the two-waves build with grids of
            // 1024 .. 2048 waves 34.2 .. 37.3 ms -- the stealing itself already fills the gaps the second wave would)
            const bool w2 = kn.two_per_simd == 1;
            // the persistent grid: as many waves as the chip holds at once (one or two per SIMD)
            p.l = {21, w2, true, kn.steal_grid > 0 ? std::min<long>(kn.steal_grid, (a.B + 2) / 3) : (w2 ? 2 * simds : simds), {}, false};
            return p;
        }
        return segments(21);
    }
    if (k > 64) {      // 65 .. 256 knots: a workgroup of two, three or four waves per problem
        p.kernel = "biconvex_admm_wg_kernel";
        const int lpp = k <= 128 ? 128 : (k <= 192 ? 192 : 256);
        // the two-waves-per-SIMD build when there are more waves than SIMDs -- and, for two waves per problem, when four such workgroups'
        // LDS fits a CU (at 127 knots only three do: 9.2 ms against 6.9 at B = 1024); four waves per problem: always (11.4-12.6 ms
        // against 15.9-16.8: tools/horizon_sweep.py)
        const bool fits = k > 128 || 4 * launch_lds_bytes(sizeof(double), 1, n_eff, a.H, (size_t)(lpp / 64) * 40) <= 160 * 1024;
        p.l = {lpp, kn.two_per_simd == 1 || (kn.two_per_simd == 2 && fits && (long)a.B * (lpp / 64) > simds), false, 0, {}, false};
        return p;
    }
    return segments(k <= 32 ? 32 : 64);
}
LaunchPlan plan_launch(const BatchArgs &a, CostShape shape, int n_eff, long simds) { return plan_launch(a, shape, n_eff, simds, g_knobs); }

hipError_t launch_biconvex_admm(const BatchArgs &args, const CostArgs &cost, int n_eff, hipStream_t stream) {
    LaunchPlan p = plan_launch(args, cost.shape, n_eff, device_simds(), g_knobs);
    if (p.status != hipSuccess || !p.kernel) return p.status;
    for (long stride : {cost.sx, cost.sf})
        if (stride < 0 || stride > (1L << 26)) return hipErrorInvalidValue;
    BatchArgs a = args;
    a.exact_step_decisions = g_knobs.exact_step_decisions;      // (every kernel with the fp32 shortcut of its step decisions; none with block or band costs)
    a.certified_steps = p.certified_steps;
    // (read by the loop-constants build alone; mode 2, "when it pays": see kForceFootPairsPay.  Results do not depend on it)
    a.force_foot_pairs = p.l.clds && (g_knobs.force_foot_pairs == 1 || (g_knobs.force_foot_pairs != 0 && kForceFootPairsPay)) ? 1 : 0;
    if (p.l.mate_rule) a.force_foot_pairs |= 2;      // (bit 1, read by the eight-wave geometry alone: its SIMD-mates keep level)
    t_last_kernel = p.kernel;
    t_last_lpp = p.l.lpp;
    t_last_block = p.latency ? 0 : (p.l.mates ? 512 : (p.l.lpp > 64 ? p.l.lpp : 64));
    // (the one-problem-per-wave kernel leaves the record of the waves per SIMD what the launch before it set: tests compare whole
    // (name, lanes, waves) records between consecutive launches, and bmpc_biconvex_plan_launch reports 0 for such a plan)
    if (p.latency) return launch_biconvex_latency(a, n_eff, stream);
    t_last_wpe = p.l.w2 ? 2 : 1;
    a.cmtab = momentum_table(stream);
    if (!a.cmtab) return hipErrorOutOfMemory;
    if (p.l.steal && !(a.queue = steal_counter(stream))) return hipErrorOutOfMemory;
#ifdef BMPC_SIMD_STAMPS
    a.simd_stamps = g_simd_stamps;
#endif
    p.l.cost = cost;
    if (cost.shape == kBand && a.H < 2) { p.l.cost.f = nullptr; p.l.cost.sf = 0; }      // (one force knot: no pair)
    return admm_unit(cost.shape, a.precision, n_eff).launch(a, p.l, stream);
}

hipError_t launch_lane_selftest(const double *in, double *out, hipStream_t stream) {
    hipLaunchKernelGGL(lane_selftest_kernel, dim3(1), dim3(64), 0, stream, in, out);
    return hipGetLastError();
}

const char *biconvex_kernel_name(int H, int raw) {
    (void)raw;
    const int k = H + 1;
    return k <= 16 ? "biconvex_admm_kernel<double, 16" : (k <= 21 && g_knobs.three_per_wave == 1 ? "biconvex_admm_kernel<double, 21" : (k <= 32 ? "biconvex_admm_kernel<double, 32" : "biconvex_admm_kernel<double, 64"));
}

#ifdef BMPC_SIMD_STAMPS
void set_simd_stamps(unsigned long long *buf) { g_simd_stamps = buf; }
#endif

}  // namespace bunmpc

// Exported, declared in no header of include/ (as bmpc_probe_quad_screen is): the switch of the eight-wave geometry and, for its tests,
// the block size of the calling thread's latest launch.  tests/test_simd_mates_gpu.py and tools/simd_mates_stamps.py bind them.
extern "C" int bmpc_set_simd_mate_balance(int mode) { return bunmpc::set_simd_mate_balance(mode); }
extern "C" int bmpc_biconvex_last_block_size(void) { return bunmpc::biconvex_last_block_size(); }

#ifdef BMPC_SIMD_STAMPS
// The diagnostic build alone (BUNMPC_EXTRA_FLAGS=-DBMPC_SIMD_STAMPS, tools/simd_mates_stamps.py): a device array of 8 words per wave of
// the next launches of the loop-constants build, or null for none.  The caller sizes it for the batch's waves.
extern "C" void bmpc_simd_stamps_buffer(void *device_words) { bunmpc::set_simd_stamps(static_cast<unsigned long long *>(device_words)); }
#endif
