// Contact-conditioned goals on the device (include/bunmpc_goals.h): what the reference builds where a contact-conditioned policy is
// deployed (ISL/examples/iterative_algorithm/simulation.py:999-1006) -- ContactPlanner.get_contact_schedule
// (contact_planner.py:35-59, 61-256: a Raibert plan over the episode, its switches, the per-foot schedule of utils.py:104-120),
// utils.get_estimated_com (utils.py:187-219) and utils.construct_cc_goal (utils.py:36-102) -- for a whole batch in HBM.  Same
// operations in the same order as tests/cc_goal_np.py (the numpy restatement the tests compare with, bit for bit) and
// bunmpc_amd/contact_planner.py / goals.py (the host path).
//
// The walk is the walk of plan_gen.hip's plan_feet_kernel (same Raibert rule, same round(t, 3), same 1e-4 phase slack, vtrack = v_des)
// over H_cp knots that are all gait_dt long; it is restated here and not shared, so that kernel's code object stays as it is.
//   front end  one thread per problem: kinematics of x = [q, v] -> CoM, feet, hips, yaw-rotated hip offsets
//   walk       one thread per (problem, foot): the knots, that foot's events; the plan itself only where the caller asks for it
//   rows       one thread per problem: N_total, end_time, start_step, the number of goal rows and the status bits
//   goals      one thread per (problem, row, slot)
// Branchy fp64 / integer work: at episode_length = 3000 a walk thread makes 1200-1440 sequential knot steps; nothing to stage.
#include <cmath>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/bunmpc.h"
#include "../../include/bunmpc_goals.h"
#include "ik_types.h"
#include "rbd_quad.h"

// bit-for-bit agreement with the numpy restatement needs separate multiplies and adds (no fused contraction)
#pragma clang fp contract(off)

namespace bunmpc {
int set_error(int code, const std::string &msg);
int model_on_device(const void *model, int *nframes, const RobotModelDev **dev);      // bunmpc_ik_capi.hip
namespace {

constexpr double kGravity = 9.81, kFootSize = 0.018;   // contact_planner.py:17-18
constexpr double kSwitchZ = 1e-3;                      // contact_planner.py:53

__device__ __forceinline__ double round3(double x) { return rint(x * 1000.0) / 1000.0; }   // np.round(x, 3)

__device__ __forceinline__ double gait_phi(double t, double period, double offset) { return fmod(t + offset * period, period); }
__device__ __forceinline__ double gait_phase(double t, double period, double sp, double offset) {   // gait_planner.cpp:46-58
    const double st = period * sp, phi = gait_phi(t, period, offset);
    return (phi <= st || fabs(phi - st) < 1e-4) ? 1.0 : 0.0;
}
__device__ __forceinline__ double gait_percent(double t, double period, double sp, double offset) {   // gait_planner.cpp:112-128
    const double st = period * sp, phi = gait_phi(t, period, offset);
    return phi <= st ? phi / st : (phi - st) / (period - st);
}

// contact_planner.py:80-124: offsets[j] = round(hip_j - com, 3), y widened, R(q)^T offsets[j]; the planning rotation is yaw only
__global__ void cc_front_kernel(const RobotModelDev *model, const bmpc_cc_goal_wb_batch_t d) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= d.g.B) return;
    const double *x = d.x + b * kNX;
    rbd::Pass1 p1;
    const int fid[kFrameSlots] = {d.foot_frame[0], d.foot_frame[1], d.foot_frame[2], d.foot_frame[3]};
    rbd::quad_pass1<false>(*model, x, fid, p1);
    double com[3], Rb[9];
    for (int c = 0; c < 3; ++c) { com[c] = p1.com[c]; d.com[b * 3 + c] = com[c]; }
    for (int c = 0; c < 9; ++c) Rb[c] = p1.Rb[c];
    for (int j = 0; j < 4; ++j) for (int c = 0; c < 3; ++c) d.feet0[(b * 4 + j) * 3 + c] = p1.fx[j][c];
    const int hid[kFrameSlots] = {d.hip_frame[0], d.hip_frame[1], d.hip_frame[2], d.hip_frame[3]};
    rbd::quad_pass1<false>(*model, x, hid, p1);
    const double yaw = atan2(Rb[3], Rb[0]), cy = cos(yaw), sy = sin(yaw);       // matrixToRpy, roll = pitch = 0 (:121-124)
    for (int j = 0; j < 4; ++j) {
        double o[3];
        for (int c = 0; c < 3; ++c) { d.hips[(b * 4 + j) * 3 + c] = p1.fx[j][c]; o[c] = round3(p1.fx[j][c] - com[c]); }
        o[1] += (j & 1) ? -0.04 : 0.04;                                          // FL, FR, HL, HR (:100-110)
        const double ox = Rb[0] * o[0] + Rb[3] * o[1] + Rb[6] * o[2];            // R^T o (:119)
        const double oy = Rb[1] * o[0] + Rb[4] * o[1] + Rb[7] * o[2];
        d.hip_off[(b * 4 + j) * 2] = cy * ox - sy * oy;                          // (R_yaw offsets[j])[0:2] (:188)
        d.hip_off[(b * 4 + j) * 2 + 1] = sy * ox + cy * oy;
    }
}

__global__ void cc_walk_kernel(const bmpc_cc_goal_batch_t d) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)d.B * 4) return;
    const long b = id / 4;
    const int j = (int)(id % 4), H = d.n_knots, cap = d.max_events;
    const double sp = d.gait.stance_percent[j], off = d.gait.phase_offset[j], gdt = d.gait.gait_dt, period = d.gait.gait_period;
    const double t0 = d.t0[b], wdes = d.w_des[b];
    const double vx = d.v_des[b * 3], vy = d.v_des[b * 3 + 1];
    const double cx = round3(d.com[b * 3]), cy = round3(d.com[b * 3 + 1]), zh = d.com[b * 3 + 2];     // :85-86
    const double hx = d.hip_off[(b * 4 + j) * 2], hy = d.hip_off[(b * 4 + j) * 2 + 1];
    // np.cross(0.5 sqrt(z/g) vtrack, [0,0,w]) -> (a_y w, -a_x w)      (:194-195)
    const double kz = 0.5 * sqrt(zh / kGravity);
    const double angx = (kz * vy) * wdes, angy = -(kz * vx) * wdes;
    // raibert = 0.5 vtrack period sp - 0.05 (vtrack - v_des): vtrack = v_des (:126, :191)
    const double rbx = 0.5 * vx * period * sp - 0.05 * (vx - vx), rby = 0.5 * vy * period * sp - 0.05 * (vy - vy);
    const double step0 = t0 / d.sim_dt;                        // get_switches(cnt_plan, start_time / sim_dt) (:254)
    const bool plan = d.cnt_plan != nullptr;
    double *cp = plan ? d.cnt_plan + (b * H * 4 + j) * 4 : nullptr;     // stride 16 doubles per knot
    double *sw = plan ? d.swing_time + b * H * 4 + j : nullptr;         // stride 4 per knot
    double *ev = d.schedule + (b * 4 + j) * (long)cap * 4;
    int n = 0;
    double pflag = gait_phase(t0, period, sp, off);
    double px = round3(d.feet0[(b * 4 + j) * 3]), py = round3(d.feet0[(b * 4 + j) * 3 + 1]), pz = round3(d.feet0[(b * 4 + j) * 3 + 2]);
    if (plan) { cp[0] = pflag; cp[1] = px; cp[2] = py; cp[3] = pz; sw[0] = 0.0; }
    for (int i = 1; i < H; ++i) {
        const double ft = round3(t0 + i * gdt);
        const double ph = gait_phase(ft, period, sp, off);
        const double hipx = cx + hx + i * gdt * vx, hipy = cy + hy + i * gdt * vy;
        const double per = round3(gait_percent(ft, period, sp, off));
        double x, y, z, s = 0.0;
        if (ph == 1.0) {
            if (pflag == 1.0) { x = px; y = py; z = pz; }
            else {
                x = rbx + hipx + angx; y = rby + hipy + angy; z = kFootSize;
                if (n < cap) { double *e = ev + 4L * n; e[0] = step0 + i * gdt / d.sim_dt; e[1] = x; e[2] = y; e[3] = kSwitchZ; }   // :51-53
                ++n;
            }
        } else {
            if (per < 0.5) { x = hipx + angx; y = hipy + angy; }
            else { x = hipx + angx + rbx; y = hipy + angy + rby; }
            z = kFootSize;
            s = (per - 0.5 < 0.02) ? 1.0 : 0.0;
        }
        if (plan) {
            double *c = cp + (long)i * 16;
            c[0] = ph; c[1] = x; c[2] = y; c[3] = z;
            sw[(long)i * 4] = s;
        }
        pflag = ph; px = x; py = y; pz = z;
    }
    for (int k = n < cap ? n : cap; k < cap; ++k) { double *e = ev + 4L * k; e[0] = e[1] = e[2] = e[3] = 0.0; }
    d.counts[b * 4 + j] = n;
}

// utils.py:52-57 and the index of :63-66 over a problem's rows.  A foot's event times grow with the knot, so the reference's scan
// (ee_contact_index) gives sw + 1 on [s[sw], s[sw + 1]) and 0 before the first event; rows end before every foot's last event.
__global__ void cc_rows_kernel(const bmpc_cc_goal_batch_t d) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= d.B) return;
    const int cap = d.max_events;
    int c[4], N = 0;
    for (int e = 0; e < 4; ++e) { c[e] = d.counts[b * 4 + e]; N += c[e]; }
    int status = 0, rows = 0;
    if (N > cap) status = BMPC_CC_EVENTS_OVERFLOW;
    else if (N < 2) status = BMPC_CC_FEW_SWITCHES;
    else {
        int end = d.episode_length + 1;                                   // simulation.py:1005
        for (int e = 0; e < 4; ++e) {
            const double *s = d.schedule + (b * 4 + e) * (long)cap * 4;
            double m = c[e] < N ? 0.0 : s[0];                             // np.max of the row: its events and, with fewer than N_total, zeros
            for (int k = 0; k < c[e]; ++k) m = fmax(m, s[4L * k]);
            end = (int)fmin((double)end, m);
        }
        const int start = (int)(d.t0[b] / d.sim_dt);                      // simulation.py:996
        if (start >= end) status = BMPC_CC_START_AFTER_END;
        else {
            const int n = end - start;
            int bad = n;
            if (d.goal_horizon - 1 >= N) bad = 0;
            else for (int e = 0; e < 4; ++e) {
                const double *s = d.schedule + (b * 4 + e) * (long)cap * 4;
                for (int k = 0; k + 1 < c[e]; ++k) {
                    if (k + d.goal_horizon < N) continue;                 // index k + 1, slot gh = goal_horizon - 1
                    const double lo = ceil(s[4L * k]), hi = ceil(s[4L * (k + 1)]);
                    const int tlo = lo > (double)start ? (int)lo : start, thi = hi < (double)end ? (int)hi : end;
                    if (tlo < thi && tlo - start < bad) bad = tlo - start;
                }
            }
            if (bad < n) status = BMPC_CC_PAST_SCHEDULE;
            rows = bad < d.max_rows ? bad : d.max_rows;
            if (rows < 0) rows = 0;
        }
    }
    d.rows[b] = rows;
    d.status[b] = status;
}

__global__ void cc_goal_kernel(const bmpc_cc_goal_batch_t d) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int S = 4 * d.goal_horizon;
    const long per = (long)d.max_rows * S;
    if (id >= (long)d.B * per) return;
    const long b = id / per;
    const int row = (int)((id % per) / S), slot = (int)(id % S), gh = slot / 4, e = slot % 4;
    double *out = d.goals + id * 3;
    if (row >= d.rows[b]) { out[0] = out[1] = out[2] = 0.0; return; }
    const int t = (int)(d.t0[b] / d.sim_dt) + row;
    const int cnt = min(d.counts[b * 4 + e], d.max_events);
    const double *s = d.schedule + (b * 4 + e) * (long)d.max_events * 4;
    int idx = 0;                                                          // ee_contact_index (utils.py:87-102); the zero padding never holds t >= 0
    for (int k = 0; k + 1 < cnt; ++k)
        if ((double)t >= s[4L * k] && (double)t < s[4L * (k + 1)]) { idx = k + 1; break; }
    const int k = idx + gh;
    const bool real = k < cnt;                                            // from the foot's count up to N_total - 1: the array's zeros
    const double e0 = real ? s[4L * k] : 0.0, e1 = real ? s[4L * k + 1] : 0.0, e2 = real ? s[4L * k + 2] : 0.0;
    double cx, cy;
    if (d.com_rows) { cx = d.com_rows[(b * d.max_rows + row) * 3]; cy = d.com_rows[(b * d.max_rows + row) * 3 + 1]; }
    else {                                                                // get_estimated_com (utils.py:209-217)
        cx = round3(d.com[b * 3]) + row * d.sim_dt * d.v_des[b * 3];
        cy = round3(d.com[b * 3 + 1]) + row * d.sim_dt * d.v_des[b * 3 + 1];
    }
    out[0] = 1.0 * (e0 - (double)t);                                      // base_wrt_goal forces sim_dt = 1.0 (utils.py:82-83)
    out[1] = cx - e1;
    out[2] = cy - e2;
}

bool positive(double v) { return std::isfinite(v) && v > 0.0; }

int check_batch(const bmpc_cc_goal_batch_t *d, bool arrays) {
    if (!d) return set_error(BMPC_BAD_ARG, "null goal descriptor (bmpc_cc_goal_batch_t)");
    if (d->n_eff != 4) return set_error(BMPC_BAD_ARG, "cc goals are built for n_eff = 4, got " + std::to_string(d->n_eff));
    if (d->B < 0 || d->B > (1 << 20)) return set_error(BMPC_BAD_ARG, "B must be in [0, 2^20], got " + std::to_string(d->B));
    if (d->episode_length < 1 || d->episode_length > (1 << 20))
        return set_error(BMPC_BAD_ARG, "episode_length must be in [1, 2^20], got " + std::to_string(d->episode_length));
    if (d->goal_horizon < 1 || d->goal_horizon > 64) return set_error(BMPC_BAD_ARG, "goal_horizon must be in [1, 64], got " + std::to_string(d->goal_horizon));
    if (d->max_rows < 1 || d->max_rows > (1 << 20)) return set_error(BMPC_BAD_ARG, "max_rows must be in [1, 2^20], got " + std::to_string(d->max_rows));
    if (d->max_events < 2 || d->max_events > (1 << 16))
        return set_error(BMPC_BAD_ARG, "max_events must be in [2, 2^16] (a schedule has two switches at least), got " + std::to_string(d->max_events));
    const bmpc_cc_gait_t &g = d->gait;
    if (!positive(d->sim_dt) || !positive(g.gait_period) || !positive(g.gait_dt) || !positive(g.gait_horizon))
        return set_error(BMPC_BAD_ARG, "sim_dt, gait_period, gait_dt and gait_horizon must be finite and > 0");
    for (int j = 0; j < 4; ++j)
        if (!(g.stance_percent[j] > 0.0 && g.stance_percent[j] <= 1.0) || !std::isfinite(g.phase_offset[j]))
            return set_error(BMPC_BAD_ARG, "stance percents must be in (0, 1] and phase offsets finite");
    const int H = bmpc_cc_goal_plan_knots(d->episode_length, d->sim_dt, g.gait_horizon, g.gait_period, g.gait_dt);
    if (H < 1 || H > (1 << 20)) return set_error(BMPC_BAD_ARG, "the plan needs between 1 and 2^20 knots, these sizes give " + std::to_string(H));
    if (d->n_knots != H)
        return set_error(BMPC_BAD_ARG, "n_knots must be bmpc_cc_goal_plan_knots(...) = " + std::to_string(H) + ", got " + std::to_string(d->n_knots));
    const double limit = 1099511627776.0;      // 2^40 bytes
    if ((double)d->B * d->max_rows * 12.0 * d->goal_horizon * 8.0 > limit || (double)d->B * 16.0 * d->max_events * 8.0 > limit ||
        (double)d->B * H * 16.0 * 8.0 > limit)
        return set_error(BMPC_BAD_ARG, "goals, schedule or plan of more than 2^40 bytes");
    if (!d->t0 || !d->v_des || !d->w_des) return set_error(BMPC_BAD_ARG, "missing input array (t0, v_des, w_des)");
    if (arrays && (!d->com || !d->feet0 || !d->hip_off)) return set_error(BMPC_BAD_ARG, "missing input array (com, feet0, hip_off)");
    if (!d->goals || !d->rows || !d->status || !d->schedule || !d->counts)
        return set_error(BMPC_BAD_ARG, "missing output array (goals, rows, status, schedule, counts)");
    if (!d->cnt_plan != !d->swing_time) return set_error(BMPC_BAD_ARG, "cnt_plan and swing_time: both or neither");
    return BMPC_OK;
}

int launch_goals(const bmpc_cc_goal_batch_t &d, hipStream_t st, const char *what) {
    const long nf = (long)d.B * 4, ng = (long)d.B * d.max_rows * 4 * d.goal_horizon;
    hipLaunchKernelGGL(cc_walk_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, d);
    hipLaunchKernelGGL(cc_rows_kernel, dim3((unsigned)((d.B + 63) / 64)), dim3(64), 0, st, d);
    hipLaunchKernelGGL(cc_goal_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, st, d);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(BMPC_DEVICE_ERROR, std::string(what) + hipGetErrorString(e));
    return BMPC_OK;
}

}  // namespace
}  // namespace bunmpc

extern "C" int bmpc_cc_goal_plan_knots(int episode_length, double sim_dt, double gait_horizon, double gait_period, double gait_dt) {
    const double h = 20.0 * episode_length * sim_dt * gait_horizon * gait_period / gait_dt;      // contact_planner.py:130
    if (!(h >= 0.0) || h > 1073741824.0) return -1;
    return (int)h;
}
extern "C" int bmpc_cc_goal_batch_struct_size(void) { return (int)sizeof(bmpc_cc_goal_batch_t); }
extern "C" int bmpc_cc_goal_wb_batch_struct_size(void) { return (int)sizeof(bmpc_cc_goal_wb_batch_t); }

extern "C" int bmpc_cc_goal_batch_device(const bmpc_cc_goal_batch_t *d, void *hip_stream) {
    using namespace bunmpc;
    if (int rc = check_batch(d, true)) return rc;
    if (d->B == 0) return BMPC_OK;
    return launch_goals(*d, static_cast<hipStream_t>(hip_stream), "cc goal kernels: ");
}

extern "C" int bmpc_cc_goal_wb_batch_device(const bmpc_cc_goal_wb_batch_t *d, void *hip_stream) {
    using namespace bunmpc;
    if (!d) return set_error(BMPC_BAD_ARG, "null goal descriptor (bmpc_cc_goal_wb_batch_t)");
    if (int rc = check_batch(&d->g, false)) return rc;
    if (!d->model) return set_error(BMPC_BAD_ARG, "null model");
    if (!d->x) return set_error(BMPC_BAD_ARG, "missing input array (x)");
    if (!d->com || !d->feet0 || !d->hips || !d->hip_off) return set_error(BMPC_BAD_ARG, "missing intermediate array (com, feet0, hips, hip_off)");
    int nframes = 0;
    const RobotModelDev *model = nullptr;
    if (int rc = model_on_device(d->model, &nframes, nullptr)) return rc;
    for (int j = 0; j < 4; ++j)
        if (d->foot_frame[j] < 0 || d->foot_frame[j] >= nframes || d->hip_frame[j] < 0 || d->hip_frame[j] >= nframes)
            return set_error(BMPC_BAD_ARG, "foot or hip frame out of range: the model has " + std::to_string(nframes) + " frames");
    if (d->g.B == 0) return BMPC_OK;
    if (int rc = model_on_device(d->model, &nframes, &model)) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(cc_front_kernel, dim3((unsigned)((d->g.B + 63) / 64)), dim3(64), 0, st, model, *d);
    bmpc_cc_goal_batch_t g = d->g;
    g.com = d->com; g.feet0 = d->feet0; g.hip_off = d->hip_off;
    return launch_goals(g, st, "whole-body cc goal kernels: ");
}
