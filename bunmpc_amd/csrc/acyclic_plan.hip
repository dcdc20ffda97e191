// Acyclic motions on the device (include/ext/bunmpc_acyclic.h): what SoloAcyclicGen.create_contact_plan / create_costs build per MPC
// call on the host (ISL/examples/mpc/abstract_acyclic_gen.py:74-296) -- the rows of a motion's time tables that hold at every knot time:
// contact plan, nominal centroidal states, bounds, swing targets, state / control regularisation -- and the zero-order-hold 1 kHz
// expansion of its optimize (:331-345), for a whole batch in HBM.  Same operations in the same order as bunmpc_amd/acyclic_gen.py
// (tests/acyclic_np.py packs what that mirror hands its solver objects; the tests compare whole arrays, bit for bit): two time walks
// with their different rounding, the first-knot dt rule on the absolute time, last rows held past a table's end, zeros before it.
//
//   state   the centroidal state of x = [q, v]: the kernel of bmpc_ik_centroidal_state_device (ik_ddp.hip), the one the solve starts from
//   nodes   one thread per (problem, node): its two knot times (a rounded prefix of at most 255 steps, recomputed per thread), the
//           look-ups, and every output entry of that node -- nothing outside its block
//   hold    one thread per (problem, output row, component)
// Branchy fp64 work on tables of a few hundred doubles that stay in cache; HBM-bound at ~(16 + 2 + 9 + 6 + 33 + 36 + 37 + 18) doubles
// written per node.  No table content becomes an index: the row counts are the struct's ints, checked on the host.
#include <cmath>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/bunmpc.h"
#include "../../include/ext/bunmpc_acyclic.h"
#include "ik_types.h"

// bit-for-bit agreement with the numpy mirror needs separate multiplies and adds (no fused contraction)
#pragma clang fp contract(off)

namespace bunmpc {
int set_error(int code, const std::string &msg);
int model_on_device(const void *model, int *nframes, const RobotModelDev **dev);      // bunmpc_ik_capi.hip
namespace {

__device__ __forceinline__ double round3(double x) { return rint(x * 1000.0) / 1000.0; }   // np.round(x, 3)
__device__ __forceinline__ double round2(double x) { return rint(x * 100.0) / 100.0; }

// np.remainder(a, b): the sign of b (numpy's npy_divmod)
__device__ __forceinline__ double np_remainder(double a, double b) {
    double mod = fmod(a, b);
    if (b == 0.0) return mod;
    if (mod != 0.0) { if ((b < 0.0) != (mod < 0.0)) mod += b; }
    else mod = copysign(0.0, b);
    return mod;
}

// A table look-up of the mirror: `n` rows of `stride` doubles with [start, end) at row[lo], row[hi]; `end` the last row's end time.
// ft < end: the first row that holds ft, or -1 (the mirror leaves zeros / adds no cost); otherwise `past` (n - 1: the last row is held;
// -1: nothing, the swing tasks).  A NaN ft fails ft < end and takes `past`, as in the mirror.
__device__ __forceinline__ int table_row(const double *tab, int n, int stride, int lo, int hi, double end, double ft, int past) {
    if (ft < end) {
        for (int k = 0; k < n; ++k)
            if (tab[k * stride + lo] <= ft && ft < tab[k * stride + hi]) return k;
        return -1;
    }
    return past;
}

__global__ void acyclic_nodes_kernel(const bmpc_acyclic_plan_t d) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int H = d.n_col, nn = H + 1;
    if (id >= (long)d.B * nn) return;
    const long b = id / nn;
    const int i = (int)(id % nn);
    const double t = d.t[b], t0 = d.t0[b], dt0 = d.dt_arr[0];
    // the two walks up to this node (:76-80 and _knot_times)
    double fc = round3(t - dt0 - t0), fk = t - dt0 - t0;
    for (int k = 0; k <= i; ++k) {
        const double dk = d.dt_arr[min(k, H - 1)];
        if (k < H) fc += round3(dk);
        fk = round3(fk + dk);
    }
    double *tk = d.ik_tasks + id * kNodeTaskDoubles;
    for (int c = 0; c < kNodeTaskDoubles; ++c) tk[c] = 0.0;
    tk[5 * kFrameSlots] = d.cent_wt[0];
    tk[5 * kFrameSlots + 4] = d.cent_wt[1];

    if (i < H) {
        const long kn = b * H + i;
        // contact plan (:74-122)
        double *cp = d.cnt_plan + kn * 16;
        const int kc = table_row(d.tab_cnt_plan, d.n_cnt, 24, 4, 5, d.tab_cnt_plan[(d.n_cnt - 1) * 24 + 5], fc, d.n_cnt - 1);
        for (int j = 0; j < 4; ++j)
            for (int c = 0; c < 4; ++c) cp[4 * j + c] = kc < 0 ? 0.0 : d.tab_cnt_plan[kc * 24 + 6 * j + c];
        d.dt_ik[kn] = d.dt_arr[i];
        if (i == 0) {      // first-knot rule on the absolute time (:110-115)
            const double dd = dt0 - round2(np_remainder(t, dt0));
            d.dt[kn] = dd == 0.0 ? dt0 : dd;
        } else d.dt[kn] = d.dt_arr[i];
        // nominal centroidal states (:127-160); knot 0 is the current state (:185)
        const int kx = table_row(d.tab_X_nom, d.n_x, 11, 9, 10, d.tab_X_nom[(d.n_x - 1) * 11 + 10], fk, -2);
        double *xn = d.X_nom + kn * 9;
        for (int c = 0; c < 9; ++c) {
            const double v = kx == -2 ? d.tab_X_ter[c] : kx < 0 ? 0.0 : d.tab_X_nom[kx * 11 + c];
            xn[c] = i == 0 ? d.x_init[b * 9 + c] : v;
            if (i == H - 1) d.X_ter[b * 9 + c] = v;
        }
        // bounds (:163-181)
        const int kb = table_row(d.tab_bounds, d.n_b, 8, 6, 7, d.tab_bounds[(d.n_b - 1) * 8 + 7], fk, d.n_b - 1);
        for (int c = 0; c < 6; ++c) d.bounds[kn * 6 + c] = kb < 0 ? 0.0 : d.tab_bounds[kb * 8 + c];
        // frame tasks: contacts, then the swing window's feet (:193-222); the first four are kept
        int slots = 0, wanted = 0;
        for (int j = 0; j < 4; ++j) {
            if (cp[4 * j] == 1.0) {
                if (slots < kFrameSlots) {
                    double *s = tk + 5 * slots++;
                    s[0] = d.cnt_wt; s[1] = (double)d.foot_frame[j]; s[2] = cp[4 * j + 1]; s[3] = cp[4 * j + 2]; s[4] = cp[4 * j + 3];
                }
                ++wanted;
            }
        }
        if (d.n_sw > 0) {
            const int ks = table_row(d.tab_swing_wt, d.n_sw, 24, 4, 5, d.tab_swing_wt[(d.n_sw - 1) * 24 + 5], fk, -1);
            for (int j = 0; j < 4 && ks >= 0; ++j) {
                const double *w = d.tab_swing_wt + ks * 24 + 6 * j;
                if (w[0] > 0.0) {
                    if (slots < kFrameSlots) {
                        double *s = tk + 5 * slots++;
                        s[0] = w[0]; s[1] = (double)d.foot_frame[j]; s[2] = w[1]; s[3] = w[2]; s[4] = w[3];
                    }
                    ++wanted;
                }
            }
        }
        if (wanted > kFrameSlots) atomicOr(d.status + b, BMPC_ACY_FRAME_SLOTS);
    }
    // state regularisation, node by node, the terminal node too (:229-250)
    const int ks = table_row(d.tab_state_scale, d.n_s, 3, 1, 2, d.state_end, fk, d.n_s - 1);
    double *sw = d.state_w + id * kNDX, *xr = d.x_reg + id * kNX;
    for (int c = 0; c < kNDX; ++c) sw[c] = ks < 0 ? 0.0 : d.tab_state_wt[ks * kNDX + c];
    for (int c = 0; c < kNX; ++c) xr[c] = ks < 0 ? (c == 6 ? 1.0 : 0.0) : d.tab_state_reg[ks * kNX + c];
    tk[5 * kFrameSlots + 11] = ks < 0 ? 0.0 : d.tab_state_scale[ks * 3];
    // control regularisation: ctrl_wt[k][0] on the running nodes, ctrl_scale[k][0] on the terminal one (:262, 277)
    const int kq = table_row(d.tab_ctrl_scale, d.n_c, 3, 1, 2, d.tab_ctrl_scale[(d.n_c - 1) * 3 + 2], fk, d.n_c - 1);
    if (i < H) {
        double *cw = d.ctrl_w + (b * H + i) * kNV;
        for (int c = 0; c < kNV; ++c) cw[c] = kq < 0 ? 0.0 : d.tab_ctrl_wt[kq * kNV + c];
        tk[5 * kFrameSlots + 12] = kq < 0 ? 0.0 : d.tab_ctrl_wt[kq * kNV];
    } else tk[5 * kFrameSlots + 12] = kq < 0 ? 0.0 : d.tab_ctrl_scale[kq * 3];
}

// int(dt / step) of the mirror; what is no positive count (negative, NaN) gives no row, and the count is capped before the conversion
__device__ __forceinline__ int hold_count(double dt, double step) {
    const double q = dt / step;
    return q >= 1.0 ? (q < 1073741824.0 ? (int)q : 1073741824) : 0;
}

__global__ void hold_kernel(const bmpc_hold_batch_t d) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = (long)d.max_rows * d.width;
    if (id >= (long)d.B * per) return;
    const long b = id / per;
    const int row = (int)((id % per) / d.width), c = (int)(id % d.width);
    const double *dt = d.dt + b * d.dt_stride;
    int i = 0;
    long first = 0;
    for (; i < d.size; ++i) {                      // which knot holds this row
        const int n = hold_count(dt[i], d.step);
        if (row < first + n) break;
        first += n;
    }
    if (c == 0 && row == 0) {
        long tot = 0;
        for (int k = 0; k < d.size; ++k) tot += hold_count(dt[k], d.step);
        d.rows[b] = (int)(tot < d.max_rows ? tot : d.max_rows);
    }
    d.out[(b * d.max_rows + row) * d.width + c] = i == d.size ? 0.0 : d.knots[(b * d.n_knots + i) * d.width + c];
}

int bad(const std::string &msg) { return set_error(BMPC_BAD_ARG, msg); }

int check_plan(const bmpc_acyclic_plan_t *d) {
    if (!d) return bad("null plan descriptor (bmpc_acyclic_plan_t)");
    if (!d->model) return bad("null model (bmpc_acyclic_plan_t.model)");
    if (d->B < 0) return bad("bmpc_acyclic_plan_t.B < 0, got " + std::to_string(d->B));
    if (d->n_col < 1 || d->n_col > 255) return bad("bmpc_acyclic_plan_t.n_col must be in [1, 255], got " + std::to_string(d->n_col));
    const struct { const char *name; int n, lo; } counts[] = {{"n_cnt", d->n_cnt, 1}, {"n_x", d->n_x, 1}, {"n_b", d->n_b, 1}, {"n_sw", d->n_sw, 0},
                                                              {"n_s", d->n_s, 1}, {"n_c", d->n_c, 1}};
    for (const auto &c : counts)
        if (c.n < c.lo || c.n > BMPC_ACY_MAX_PHASES)
            return bad(std::string("bmpc_acyclic_plan_t.") + c.name + " must be in [" + std::to_string(c.lo) + ", 16], got " + std::to_string(c.n));
    if (!std::isfinite(d->cnt_wt)) return bad("bmpc_acyclic_plan_t.cnt_wt must be finite");
    if (!std::isfinite(d->cent_wt[0]) || !std::isfinite(d->cent_wt[1])) return bad("bmpc_acyclic_plan_t.cent_wt must be finite");
    if (std::isnan(d->state_end)) return bad("bmpc_acyclic_plan_t.state_end must not be NaN");
    const struct { const char *name; const void *p; } arrays[] = {
        {"x", d->x}, {"t", d->t}, {"t0", d->t0}, {"dt_arr", d->dt_arr}, {"tab_cnt_plan", d->tab_cnt_plan}, {"tab_X_nom", d->tab_X_nom},
        {"tab_X_ter", d->tab_X_ter}, {"tab_bounds", d->tab_bounds}, {"tab_swing_wt", d->n_sw ? (const void *)d->tab_swing_wt : (const void *)d},
        {"tab_state_reg", d->tab_state_reg}, {"tab_state_wt", d->tab_state_wt}, {"tab_state_scale", d->tab_state_scale},
        {"tab_ctrl_wt", d->tab_ctrl_wt}, {"tab_ctrl_scale", d->tab_ctrl_scale}, {"cnt_plan", d->cnt_plan}, {"dt", d->dt}, {"dt_ik", d->dt_ik},
        {"x_init", d->x_init}, {"X_nom", d->X_nom}, {"X_ter", d->X_ter}, {"bounds", d->bounds}, {"ik_tasks", d->ik_tasks},
        {"state_w", d->state_w}, {"x_reg", d->x_reg}, {"ctrl_w", d->ctrl_w}, {"status", d->status}};
    for (const auto &a : arrays)
        if (!a.p) return bad(std::string("missing array: bmpc_acyclic_plan_t.") + a.name + " is NULL");
    int nframes = 0;
    if (int rc = model_on_device(d->model, &nframes, nullptr)) return rc;
    for (int j = 0; j < 4; ++j)
        if (d->foot_frame[j] < 0 || d->foot_frame[j] >= nframes)
            return bad("bmpc_acyclic_plan_t.foot_frame[" + std::to_string(j) + "] = " + std::to_string(d->foot_frame[j]) + " is outside the model's " +
                       std::to_string(nframes) + " frames");
    return BMPC_OK;
}

}  // namespace
}  // namespace bunmpc

extern "C" int bmpc_acyclic_plan_struct_size(void) { return (int)sizeof(bmpc_acyclic_plan_t); }
extern "C" int bmpc_hold_batch_struct_size(void) { return (int)sizeof(bmpc_hold_batch_t); }

extern "C" int bmpc_acyclic_plan_batch_device(const bmpc_acyclic_plan_t *d, void *hip_stream) {
    using namespace bunmpc;
    if (int rc = check_plan(d)) return rc;
    if (d->B == 0) return BMPC_OK;
    int nframes = 0;
    const RobotModelDev *model = nullptr;
    if (int rc = model_on_device(d->model, &nframes, &model)) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipError_t e = hipMemsetAsync(d->status, 0, sizeof(int) * (size_t)d->B, st);
    if (e == hipSuccess) e = ik_launch_centroidal_state(model, d->x, d->x_init, d->B, st);
    if (e == hipSuccess) {
        const long n = (long)d->B * (d->n_col + 1);
        hipLaunchKernelGGL(acyclic_nodes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, *d);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return set_error(BMPC_DEVICE_ERROR, std::string("acyclic plan kernels: ") + hipGetErrorString(e));
    return BMPC_OK;
}

extern "C" int bmpc_hold_batch_device(const bmpc_hold_batch_t *d, void *hip_stream) {
    using namespace bunmpc;
    if (!d) return bad("null hold descriptor (bmpc_hold_batch_t)");
    const struct { const char *name; const void *p; } arrays[] = {{"knots", d->knots}, {"dt", d->dt}, {"out", d->out}, {"rows", d->rows}};
    for (const auto &a : arrays)
        if (!a.p) return bad(std::string("missing array: bmpc_hold_batch_t.") + a.name + " is NULL");
    if (d->B < 0) return bad("bmpc_hold_batch_t.B < 0, got " + std::to_string(d->B));
    const struct { const char *name; int n; } sizes[] = {{"n_knots", d->n_knots}, {"width", d->width}, {"size", d->size}, {"max_rows", d->max_rows}};
    for (const auto &s : sizes)
        if (s.n < 1) return bad(std::string("bmpc_hold_batch_t.") + s.name + " must be >= 1, got " + std::to_string(s.n));
    if (d->size > d->n_knots) return bad("bmpc_hold_batch_t.size must be <= n_knots: every interval holds its own knot");
    if (d->dt_stride < d->size) return bad("bmpc_hold_batch_t.dt_stride must be >= size");
    if (!std::isfinite(d->step) || !(d->step > 0.0)) return bad("bmpc_hold_batch_t.step must be finite and > 0");
    if ((double)d->B * d->max_rows * d->width > 274877906944.0) return bad("bmpc_hold_batch_t: B * max_rows * width is more than 2^38 entries");
    if (d->B == 0) return BMPC_OK;
    const long n = (long)d->B * d->max_rows * d->width;
    hipLaunchKernelGGL(hold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), *d);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(BMPC_DEVICE_ERROR, std::string("hold kernel: ") + hipGetErrorString(e));
    return BMPC_OK;
}
