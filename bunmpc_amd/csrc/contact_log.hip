// Measured contact goals on the device (include/ext/bunmpc_contact_log.h): what four rollout functions of
// ISL/examples/iterative_algorithm/simulation.py do with the contacts their simulator measured (:437-438, :537-550, :563-578) -- new_ee_contact
// (:299-314) per step, the per-foot event list, utils.construct_contact_schedule (utils.py:104-120) and utils.construct_cc_goal
// (utils.py:36-102) over the measured CoM history, failed_states (:189-220) -- for B logged episodes in HBM.  bunmpc_amd/contact_log.py is
// the host path; its host_batch() is the numpy twin the tests compare with, bit for bit.
//
//   events   one workgroup (four waves) per episode.  A chunk is 256 consecutive rows, a wave's block 64 of them: the wave loads its
//            block's 768 doubles as twelve loads of 64 consecutive doubles and stages them in LDS; lane l then looks at row l: contact
//            bits (abs(x) > 1e-12) and cleared bits (abs(x) <= 1e-12: not the complement, a NaN is neither) of the four feet by
//            ballot; the cleared bit of the row before the block comes from the wave before it in LDS, for the chunk's first block
//            from the chunk before (carried in a register; "cleared" before row 0); rising edges = contact & (cleared << 1 | seam);
//            a foot's list positions = the workgroup's running count + the counts of the chunk's earlier blocks (through LDS) + the
//            population count of the edges below the lane.  Two barriers per chunk; the log is read once.
//   failed   one thread per (episode, row), a wave inside one episode: the flag, a ballot, one integer atomicMin per wave with a flag
//   rows     one thread per episode: N_total, end_time, rows, status, failed_step
//   goals    one thread per (episode, row, slot); a workgroup's slots go through LDS and are stored as consecutive doubles.  The interval
//            scan is that of cc_goals.hip's cc_goal_kernel, restated here and not shared, so that file's code object stays as it is (as
//            that file did with plan_feet_kernel).
// A stage reads what the stage before it wrote only across a kernel boundary of the stream.  The first failing row is gathered in
// status[b] (set to kNoRow by the events kernel, lowered by atomicMin, replaced by the bits in the rows kernel): no scratch memory.
// Every address is bounded by what the host passed (B, T, max_events, max_rows): counts and rows read back from device memory are
// clamped before use.
#include <cmath>
#include <cstdint>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/bunmpc.h"
#include "../../include/ext/bunmpc_contact_log.h"

// bit-for-bit agreement with the numpy twin needs separate multiplies and adds (no fused contraction)
#pragma clang fp contract(off)

namespace bunmpc {
int set_error(int code, const std::string &msg);
namespace {

constexpr int kThreads = 256, kWave = 64, kWaves = kThreads / kWave;
constexpr int kRowDoubles = 12;                       // [4][3]
constexpr int kBlockDoubles = kWave * kRowDoubles;    // a wave's block of 64 rows
constexpr double kThreshold = 1e-12;                  // simulation.py:310
constexpr int kNoRow = 0x7fffffff;
constexpr double kRadToDeg = 180.0 / 3.141592653589793;   // math.degrees multiplies by this quotient

using mask_t = unsigned long long;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// rows of episode b that the reference's loop visits: range(start_step, episode_length), at most the T logged ones
__device__ __forceinline__ int used_rows(int T, int episode_length, long start) {
    const long n = (long)episode_length - start;
    return n < 0 ? 0 : (n > T ? T : (int)n);
}

__global__ void __launch_bounds__(kThreads) cl_events_kernel(const bmpc_contact_log_t d) {
    __shared__ double stage[kWaves][kBlockDoubles];
    __shared__ int cnt[kWaves][4];
    const int tid = threadIdx.x, w = tid / kWave, lane = tid & (kWave - 1);
    const long b = blockIdx.x;
    const int cap = d.max_events;
    const long start = d.start_step[b];
    const int n = used_rows(d.T, d.episode_length, start);
    const double *log = d.ee_pos + b * ((long)d.T * kRowDoubles);
    double *sched = d.schedule + b * 4 * (long)cap * 4;
    const long n_doubles = (long)n * kRowDoubles;
    const mask_t below = lane == 0 ? 0ULL : (~0ULL >> (kWave - lane));
    int run[4] = {0, 0, 0, 0};               // events of foot j in the chunks before this one (the same in every thread)
    unsigned carry = 0xf;                    // cleared bits of the row before the chunk: pre = 0 before row 0
    for (int row0 = 0; row0 < n; row0 += kThreads) {
        const long e0 = (long)(row0 + w * kWave) * kRowDoubles;
        double v[kRowDoubles];
#pragma unroll
        for (int i = 0; i < kRowDoubles; ++i) {
            const long e = e0 + i * kWave + lane;
            v[i] = e < n_doubles ? log[e] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < kRowDoubles; ++i) stage[w][i * kWave + lane] = v[i];
        __syncthreads();
        const int r = row0 + w * kWave + lane;
        const long o0 = start + row0 + w * kWave;      // the step of the block's first row
        const double *mine = stage[w] + lane * kRowDoubles;
        const double *last3 = stage[kWaves - 1] + (kWave - 1) * kRowDoubles, *before = stage[w > 0 ? w - 1 : 0] + (kWave - 1) * kRowDoubles;
        mask_t edge[4];
        unsigned next_carry = 0;
        int c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double x = mine[3 * j];
            const mask_t contact = __ballot(r < n && fabs(x) > kThreshold), cleared = __ballot(fabs(x) <= kThreshold);
            const unsigned seam = w > 0 ? (fabs(before[3 * j]) <= kThreshold ? 1u : 0u) : ((carry >> j) & 1u);
            edge[j] = contact & ((cleared << 1) | seam);
            if (o0 <= 0 && o0 > -kWave) edge[j] &= ~(1ULL << (int)(-o0));   // o == 0: "we do not need the switch at initialization" (:544)
            next_carry |= (fabs(last3[3 * j]) <= kThreshold ? 1u : 0u) << j;
            c[j] = __popcll(edge[j]);
        }
        carry = next_carry;
        if (lane < 4) cnt[w][lane] = c[lane];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int at = run[j], all = 0;
            for (int k = 0; k < kWaves; ++k) {
                const int ck = cnt[k][j];
                if (k < w) at += ck;
                all += ck;
            }
            run[j] += all;
            if ((edge[j] >> lane) & 1ULL) {
                const long pos = (long)at + __popcll(edge[j] & below);
                if (pos < cap) {
                    double *e = sched + ((long)j * cap + pos) * 4;
                    e[0] = (double)(start + r);
                    e[1] = mine[3 * j];
                    e[2] = mine[3 * j + 1];
                    e[3] = mine[3 * j + 2];
                }
            }
        }
        // the next chunk's stores to stage[w] and cnt follow this chunk's reads of them: a wave's own LDS accesses are in order, and another
        // wave's row 63 and counts are read before the barrier that the owner's next stores come after
    }
    for (int j = 0; j < 4; ++j) {            // zeros behind a foot's events
        const int first = run[j] < cap ? run[j] : cap;
        double *col = sched + (long)j * cap * 4;
        for (long i = 4L * first + tid; i < 4L * cap; i += kThreads) col[i] = 0.0;
    }
    if (tid < 4) d.counts[b * 4 + tid] = run[tid];
    if (tid == 4) d.status[b] = kNoRow;      // the accumulator of the failed-state minimum; cl_rows_kernel puts the bits there
}

// simulation.py:189-220 and utils.py:7-34 on row r of episode b
__global__ void __launch_bounds__(kThreads) cl_failed_kernel(const bmpc_contact_log_t d, int rows_padded) {
    const long id = (long)blockIdx.x * kThreads + threadIdx.x;
    const long b = id / rows_padded;                                   // the same for a whole wave: rows_padded is a multiple of 64
    if (b >= d.B) return;
    const int r = (int)(id - b * rows_padded);
    const int n = used_rows(d.T, d.episode_length, d.start_step[b]);
    bool failed = false;
    if (r < d.T) {
        const double *q = d.q + (b * d.T + r) * d.s_q;
        const double h = q[2], x = q[3], y = q[4], z = q[5], qw = q[6];
        const double ysqr = y * y;
        const double t0 = 2.0 * (qw * x + y * z), t1 = 1.0 - 2.0 * (x * x + ysqr);
        const double roll = atan2(t0, t1) * kRadToDeg;
        double t2 = 2.0 * (qw * y - z * x);
        t2 = t2 > 1.0 ? 1.0 : t2;
        t2 = t2 < -1.0 ? -1.0 : t2;
        const double pitch = asin(t2) * kRadToDeg;
        if (d.angles) {
            d.angles[(b * d.T + r) * 2] = roll;
            d.angles[(b * d.T + r) * 2 + 1] = pitch;
        }
        failed = r < n && (double)r > d.grace && (h < d.z_min || h > 2.0 || fabs(roll) > d.fail_angle || fabs(pitch) > d.fail_angle);
    }
    const mask_t any = __ballot(failed);
    if (any != 0 && (int)(threadIdx.x & (kWave - 1)) == __ffsll((long long)any) - 1) atomicMin(d.status + b, r);
}

__global__ void cl_rows_kernel(const bmpc_contact_log_t d) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= d.B) return;
    const int cap = d.max_events, gh = d.goal_horizon;
    int c[4];
    long N = 0;
    for (int j = 0; j < 4; ++j) { c[j] = clampi(d.counts[b * 4 + j], 0, d.T); N += c[j]; }
    const long start = d.start_step[b];
    const double *sched = d.schedule + b * 4 * (long)cap * 4;
    int status = 0;
    long rows = 0;
    if (N > cap) status = BMPC_CL_EVENTS_OVERFLOW;
    else if (N < 2) status = BMPC_CL_FEW_SWITCHES;
    else {
        long end = d.episode_length;
        for (int j = 0; j < 4; ++j) {
            // np.max of the column: a foot's steps grow along its list, so its last event, and with fewer than N_total events the zeros
            double m = c[j] > 0 ? sched[((long)j * cap + c[j] - 1) * 4] : 0.0;
            if (c[j] < N && m < 0.0) m = 0.0;
            if (m < (double)end) end = (long)m;                       // int(min(end_time, max_time)) (utils.py:55)
        }
        if (start > end) status = BMPC_CL_START_AFTER_END;
        else {
            const long n = end - start;
            long bad = n;
            if (n > 0 && gh - 1 >= N) bad = 0;
            else if (n > 0) {
                // index k + 1 on [s[k], s[k + 1]) for k + 1 < c[j] (ee_contact_index); slot gh - 1 reads k + gh >= N_total: IndexError
                for (int j = 0; j < 4; ++j) {
                    const double *s = sched + (long)j * cap * 4;
                    for (long k = N - gh; k + 1 < c[j]; ++k) {
                        const long lo = (long)s[4 * k], hi = (long)s[4 * (k + 1)];
                        const long tlo = lo > start ? lo : start, thi = hi < end ? hi : end;
                        if (tlo < thi) {
                            if (tlo - start < bad) bad = tlo - start;
                            break;
                        }
                    }
                }
            }
            if (bad < n) status = BMPC_CL_PAST_SCHEDULE;
            rows = bad < d.max_rows ? bad : d.max_rows;
        }
    }
    const int first = d.status[b];                                    // kNoRow, or the first failing row
    int failed_step = -1;
    if (d.check_failed && first != kNoRow) {
        failed_step = clampi(first, 0, d.T - 1);
        status |= BMPC_CL_FAILED_STATE;
        rows = 0;
    }
    d.rows[b] = (int)rows;
    d.status[b] = status;
    if (d.failed_step) d.failed_step[b] = failed_step;
}

// A workgroup's 256 slots are 768 consecutive doubles of goals: each thread puts its slot's three values into LDS, and the workgroup
// stores them as three rounds of 256 consecutive doubles (stored slot by slot, a wave's 8-byte stores would lie 24 bytes apart).
__global__ void __launch_bounds__(kThreads) cl_goal_kernel(const bmpc_contact_log_t d) {
    __shared__ double tile[3 * kThreads];
    const long id = (long)blockIdx.x * kThreads + threadIdx.x;
    const int S = 4 * d.goal_horizon;
    const long per = (long)d.max_rows * S, total = (long)d.B * per;
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    if (id < total) {
        const long b = id / per;
        const long in = id - b * per;
        const int row = (int)(in / S), slot = (int)(in - (long)row * S), gh = slot / 4, j = slot % 4;
        if (row < clampi(d.rows[b], 0, d.max_rows)) {
            const double t = (double)((long)d.start_step[b] + row);
            const int cnt = clampi(d.counts[b * 4 + j], 0, d.max_events);
            const double *s = d.schedule + (b * 4 + j) * (long)d.max_events * 4;
            int idx = 0;                                              // ee_contact_index (utils.py:87-102); the zero padding never holds t >= 0
            for (int k = 0; k + 1 < cnt; ++k)
                if (t >= s[4L * k] && t < s[4L * (k + 1)]) { idx = k + 1; break; }
            const int k = idx + gh;
            const bool real = k < cnt;                                // from the foot's count up to N_total - 1: the array's zeros
            const double e0 = real ? s[4L * k] : 0.0, e1 = real ? s[4L * k + 1] : 0.0, e2 = real ? s[4L * k + 2] : 0.0;
            const double *com = d.com + (b * d.T + row) * 3;
            g0 = 1.0 * (e0 - t);                                      // base_wrt_goal forces sim_dt = 1.0 (utils.py:82-83)
            g1 = com[0] - e1;
            g2 = com[1] - e2;
        }
    }
    tile[3 * threadIdx.x] = g0;
    tile[3 * threadIdx.x + 1] = g1;
    tile[3 * threadIdx.x + 2] = g2;
    __syncthreads();
    const long first = (long)blockIdx.x * (3 * kThreads);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const long e = first + i * kThreads + threadIdx.x;
        if (e < 3 * total) d.goals[e] = tile[i * kThreads + threadIdx.x];
    }
}

int bad(const std::string &msg) { return set_error(BMPC_BAD_ARG, msg); }

int check(const bmpc_contact_log_t *d) {
    if (!d) return bad("null contact log descriptor (bmpc_contact_log_t)");
    if (d->n_eff != 4) return bad("measured goals are built for n_eff = 4, got " + std::to_string(d->n_eff));
    if (d->B < 0 || d->B > (1 << 20)) return bad("B must be in [0, 2^20], got " + std::to_string(d->B));
    if (d->T < 1 || d->T > (1 << 20)) return bad("T must be in [1, 2^20], got " + std::to_string(d->T));
    if (d->episode_length < 1 || d->episode_length > (1 << 20))
        return bad("episode_length must be in [1, 2^20], got " + std::to_string(d->episode_length));
    if (d->max_rows < 1 || d->max_rows > d->T) return bad("max_rows must be in [1, T = " + std::to_string(d->T) + "], got " + std::to_string(d->max_rows));
    if (d->goal_horizon < 1 || d->goal_horizon > 64) return bad("goal_horizon must be in [1, 64], got " + std::to_string(d->goal_horizon));
    if (d->max_events < 2 || d->max_events > (1 << 16))
        return bad("max_events must be in [2, 2^16] (a schedule has two switches at least), got " + std::to_string(d->max_events));
    if (!std::isfinite(d->fail_angle)) return bad("fail_angle must be finite");
    if (!std::isfinite(d->z_min)) return bad("z_min must be finite");
    if (!std::isfinite(d->grace)) return bad("grace must be finite");
    if (d->check_failed && !d->q) return bad("null input array: q (check_failed is set)");
    if (d->q && d->s_q < 19) return bad("s_q (the row stride of q) must be 19 at least, got " + std::to_string(d->s_q));
    const double limit = 1099511627776.0, rows = (double)d->B * d->T;      // 2^40 bytes
    if (rows * kRowDoubles * 8.0 > limit) return bad("ee_pos of more than 2^40 bytes");
    if (d->q && rows * (double)d->s_q * 8.0 > limit) return bad("q of more than 2^40 bytes (B T s_q doubles)");
    if ((double)d->B * d->max_rows * 12.0 * d->goal_horizon * 8.0 > limit) return bad("goals of more than 2^40 bytes");
    if ((double)d->B * 16.0 * d->max_events * 8.0 > limit) return bad("schedule of more than 2^40 bytes");
    // one thread per goal slot and, with the failed-state test, per row of the padded log: a launch takes fewer than 2^32 threads
    const double threads = 4294967296.0;
    if ((double)d->B * d->max_rows * 4.0 * d->goal_horizon >= threads)
        return bad("B max_rows 4 goal_horizon (one thread per goal slot) must be below 2^32, got " + std::to_string((double)d->B * d->max_rows * 4.0 * d->goal_horizon));
    if (d->check_failed && (double)d->B * ((d->T + kWave - 1) / kWave * kWave) >= threads)
        return bad("B T (one thread per row of the failed-state test, T rounded up to 64) must be below 2^32, got " + std::to_string(rows));
    if (!d->start_step) return bad("null input array: start_step");
    if (!d->ee_pos) return bad("null input array: ee_pos");
    if (!d->com) return bad("null input array: com");
    if (!d->schedule) return bad("null output array: schedule");
    if (!d->counts) return bad("null output array: counts");
    if (!d->goals) return bad("null output array: goals");
    if (!d->rows) return bad("null output array: rows");
    if (!d->status) return bad("null output array: status");
    return BMPC_OK;
}

}  // namespace
}  // namespace bunmpc

extern "C" int bmpc_contact_log_struct_size(void) { return (int)sizeof(bmpc_contact_log_t); }

extern "C" int bmpc_contact_log_goals_device(const bmpc_contact_log_t *d, void *hip_stream) {
    using namespace bunmpc;
    if (int rc = check(d)) return rc;
    if (d->B == 0) return BMPC_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const long B = d->B;
    hipLaunchKernelGGL(cl_events_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, *d);
    if (d->check_failed) {
        const int rows_padded = (d->T + kWave - 1) / kWave * kWave;
        hipLaunchKernelGGL(cl_failed_kernel, dim3((unsigned)((B * rows_padded + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, *d, rows_padded);
    }
    hipLaunchKernelGGL(cl_rows_kernel, dim3((unsigned)((B + kWave - 1) / kWave)), dim3(kWave), 0, st, *d);
    const long ng = B * d->max_rows * 4 * d->goal_horizon;
    hipLaunchKernelGGL(cl_goal_kernel, dim3((unsigned)((ng + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, *d);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(BMPC_DEVICE_ERROR, std::string("contact log kernels: ") + hipGetErrorString(e));
    return BMPC_OK;
}
