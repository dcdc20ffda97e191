// The trainers' data set on the device (include/ext/bunmpc_dataset.h): the ring buffer of ISL/examples/iterative_algorithm/database.py
// (:104-146), its input statistics (:187-213) and its normalised __getitem__ (:53-83) for buffers in HBM.  tests/dataset_np.py is the
// numpy restatement the tests compare with.
//
//   append    count     one wave per problem: rows[b] clipped, keep[b], and with drop_nonfinite a scan of the kept rows of every given group
//             chunk     one workgroup per kChunk problems: exclusive prefix inside the chunk, the chunk's total
//             offsets   one workgroup: exclusive prefix over the chunk totals, the call's total n
//             scatter   one thread per pair of elements of a problem's [R][w] block, every given group in one launch (blockIdx.y)
//             header    one thread: start, length as the row-by-row loop leaves them, n
//   moments   partial   one workgroup per kMomentRows buffer rows and group: lanes walk row * w + column, one partial per column
//             final     one workgroup per column: the partials in a fixed order, then / length (and sqrt in the second pass)
//   batch     one wave per output row: gather, normalise, concatenate
// A stage reads what the stage before it wrote only across a kernel boundary of the stream: no kernel waits for another workgroup.
// Every address is bounded by what the host passed (limit, B, R, n): start, length and the totals read back from device memory are
// clamped before use, and a ring slot is a remainder modulo limit.
#include <cmath>
#include <cstdint>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/bunmpc.h"
#include "../../include/ext/bunmpc_dataset.h"

// the statistics and the batch are held to numpy's operations one by one: no fused multiply-add
#pragma clang fp contract(off)

namespace bunmpc {
int set_error(int code, const std::string &msg);
namespace {

constexpr int kThreads = 256, kWave = 64;
constexpr int kChunk = 1024;         // problems per workgroup of the prefix (4 per thread)
constexpr int kMomentRows = 1024;    // buffer rows per workgroup of a partial sum
constexpr int kGroups = 4;           // states, actions, vc_goals, cc_goals

struct Groups {
    const double *src[kGroups];      // nullptr: the group is not given
    double *dst[kGroups];
    int w[kGroups];
};

struct Scratch {                     // byte offsets into bmpc_dataset_t.scratch, each a multiple of 16
    long counts, local, chunk_tot, chunk_off, total, part_states, part_cc, bytes;
    long nchunks, nblocks;
};

long round16(long v) { return (v + 15) & ~15L; }

Scratch scratch_layout(long limit, int w_cc, int max_problems) {
    Scratch s;
    s.nchunks = ((long)max_problems + kChunk - 1) / kChunk;
    s.nblocks = (limit + kMomentRows - 1) / kMomentRows;
    long at = 0;
    s.counts = at;      at += round16((long)max_problems * (long)sizeof(int));
    s.local = at;       at += round16((long)max_problems * (long)sizeof(long));
    s.chunk_tot = at;   at += round16(s.nchunks * (long)sizeof(long));
    s.chunk_off = at;   at += round16(s.nchunks * (long)sizeof(long));
    s.total = at;       at += 16;
    s.part_states = at; at += round16(s.nblocks * BMPC_DS_STATE_WIDTH * (long)sizeof(double));
    s.part_cc = at;     at += round16(s.nblocks * w_cc * (long)sizeof(double));
    s.bytes = at;
    return s;
}

__device__ __forceinline__ long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ bool nonfinite(double v) {
    return (__double_as_longlong(v) & 0x7ff0000000000000LL) == 0x7ff0000000000000LL;
}

// ---- append ---------------------------------------------------------------------------------------------------------------------------

__global__ void ds_count_kernel(const Groups g, int B, int R, const int *rows, const int *keep, int drop_nonfinite, int *counts) {
    const int lane = threadIdx.x & (kWave - 1);
    const long b = ((long)blockIdx.x * blockDim.x + threadIdx.x) / kWave;      // the same for a whole wave
    if (b >= B) return;
    int c = rows ? rows[b] : R;
    c = c < 0 ? 0 : (c > R ? R : c);
    if (keep && keep[b] == 0) c = 0;
    if (drop_nonfinite && c > 0) {
        bool bad = false;
        for (int k = 0; k < kGroups; ++k) {
            if (!g.src[k]) continue;
            const double *p = g.src[k] + b * ((long)R * g.w[k]);
            const int m = c * g.w[k];
            for (int i = lane; i < m; i += kWave) bad |= nonfinite(p[i]);
        }
        if (__ballot(bad) != 0) c = 0;
    }
    if (lane == 0) counts[b] = c;
}

// exclusive prefix of v over the workgroup's threads (out) and the workgroup's total; every thread of the workgroup calls it
__device__ __forceinline__ long block_exclusive(long v, long *lds, long *total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const long add = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const long incl = lds[t];
    *total = lds[kThreads - 1];
    __syncthreads();
    return incl - v;
}

__global__ void ds_chunk_kernel(int B, int R, const int *counts, long *local, long *chunk_tot) {
    __shared__ long lds[kThreads];
    const long first = (long)blockIdx.x * kChunk + 4L * threadIdx.x;
    int c[4];
    long sum = 0;
    for (int i = 0; i < 4; ++i) {
        const long b = first + i;
        int v = b < B ? counts[b] : 0;
        v = v < 0 ? 0 : (v > R ? R : v);
        c[i] = v;
        sum += v;
    }
    long total;
    long at = block_exclusive(sum, lds, &total);
    for (int i = 0; i < 4; ++i) {
        if (first + i < B) local[first + i] = at;
        at += c[i];
    }
    if (threadIdx.x == 0) chunk_tot[blockIdx.x] = total;
}

__global__ void ds_offsets_kernel(long nchunks, const long *chunk_tot, long *chunk_off, long *total_out) {
    __shared__ long lds[kThreads];
    const long per = (nchunks + kThreads - 1) / kThreads;
    const long lo = per * threadIdx.x, hi = lo + per < nchunks ? lo + per : nchunks;
    long sum = 0;
    for (long i = lo; i < hi; ++i) sum += chunk_tot[i];
    long total;
    long at = block_exclusive(sum, lds, &total);
    for (long i = lo; i < hi; ++i) {
        chunk_off[i] = at;
        at += chunk_tot[i];
    }
    if (threadIdx.x == 0) total_out[0] = total;
}

// Thread `id` of group k takes elements e0 = 2 p and e0 + 1 of problem b's [R][w] block.  Kept element e of problem b is row
// j = offset[b] + e / w of the call's n kept rows: slot (start + length + j) % limit, dropped where j < n - limit.  One 16-byte load
// where the source address allows it, one 16-byte store where the two ring elements are neighbours and the first one's address allows
// it (so never across the ring's end, a dropped row or a problem's last kept element); 8-byte accesses otherwise.
__global__ void ds_scatter_kernel(const Groups g, int B, int R, long limit, const long *header, const int *counts, const long *local,
                                  const long *chunk_off, const long *total) {
    const int k = blockIdx.y;
    if (!g.src[k]) return;
    const int w = g.w[k];
    const int epb = R * w, ppb = (epb + 1) / 2;
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)B * ppb) return;
    const int b = (int)(id / ppb);
    const int e0 = 2 * (int)(id - (long)b * ppb);
    int c = counts[b];
    c = c < 0 ? 0 : (c > R ? R : c);
    const int m = c * w;
    if (e0 >= m) return;
    const long rows_max = (long)B * R;                                   // < 2^31
    const long n = clampl(total[0], 0, rows_max);
    const long off = clampl(chunk_off[b / kChunk] + local[b], 0, rows_max - c);
    const long start = clampl(header[0], 0, limit - 1), length = clampl(header[1], 0, limit);
    const long skip = n > limit ? n - limit : 0;
    const unsigned lim = (unsigned)limit, base = (unsigned)((start + length) % limit);
    const bool two = e0 + 1 < m;
    const int r0 = e0 / w, col0 = e0 - r0 * w;
    const long j0 = off + r0;
    unsigned slot0 = base + (unsigned)(j0 % limit);                      // < 2^32: both terms are below limit < 2^31
    if (slot0 >= lim) slot0 -= lim;
    const bool last_col = col0 + 1 == w;
    const int col1 = last_col ? 0 : col0 + 1;
    const long j1 = last_col ? j0 + 1 : j0;
    unsigned slot1 = last_col ? slot0 + 1 : slot0;
    if (slot1 >= lim) slot1 -= lim;
    const bool ok0 = j0 >= skip, ok1 = two && j1 >= skip;
    const long d0 = (long)slot0 * w + col0, d1 = (long)slot1 * w + col1;
    const double *s = g.src[k] + (long)b * epb + e0;
    double v0, v1 = 0.0;
    if (two && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
        const double2 v = *reinterpret_cast<const double2 *>(s);
        v0 = v.x;
        v1 = v.y;
    } else {
        v0 = s[0];
        if (two) v1 = s[1];
    }
    double *dst = g.dst[k];
    if (ok0 && ok1 && d1 == d0 + 1 && (reinterpret_cast<uintptr_t>(dst + d0) & 15) == 0) {
        *reinterpret_cast<double2 *>(dst + d0) = make_double2(v0, v1);
    } else {
        if (ok0) dst[d0] = v0;
        if (ok1) dst[d1] = v1;
    }
}

__global__ void ds_header_kernel(long limit, long rows_max, const long *total, long *header) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const long n = clampl(total[0], 0, rows_max);
    const long start = clampl(header[0], 0, limit - 1), length = clampl(header[1], 0, limit);
    const long over = length + n > limit ? length + n - limit : 0;       // rows the loop pushes out: each moves start on by one
    header[0] = (start + over % limit) % limit;
    header[1] = length + n > limit ? limit : length + n;
    header[2] = n;
    header[3] = 0;
}

// ---- moments ----------------------------------------------------------------------------------------------------------------------------

struct Moments {                     // states, cc_goals
    const double *buf[2];
    int w[2];                        // 0: no such group
    double *part[2];                 // [nblocks][w]
    double *mean[2], *std[2];
};

// DEV false: partial sums of x; true: of (x - mean)^2.  Threads (g, c) = (v / w, v % w), v < G w with G = 256 / w rows in flight (one row
// and a loop over the columns where w > 256): thread v reads element r0 w + v of the block first, so a wave reads consecutive addresses.
template <bool DEV>
__global__ void ds_partial_kernel(const Moments m, long limit, const long *header) {
    __shared__ double lds[BMPC_DS_MAX_CC_WIDTH];
    const int k = blockIdx.y, w = m.w[k];
    if (w == 0) return;
    const long length = clampl(header[1], 0, limit);
    const long r0 = (long)blockIdx.x * kMomentRows;
    if (r0 >= length) return;                                           // (the whole workgroup)
    const long r1 = r0 + kMomentRows < length ? r0 + kMomentRows : length;
    const int G = w <= kThreads ? kThreads / w : 1;
    const double *buf = m.buf[k];
    for (int v = threadIdx.x; v < G * w; v += kThreads) {
        const int gg = v / w, c = v - gg * w;
        const double mean = DEV ? m.mean[k][c] : 0.0;
        double acc = 0.0;
#pragma unroll 4
        for (long r = r0 + gg; r < r1; r += G) {
            const double x = buf[r * w + c];
            if (DEV) {
                const double d = x - mean;
                acc += d * d;
            } else {
                acc += x;
            }
        }
        lds[v] = acc;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < w; c += kThreads) {
        double s = 0.0;
        for (int gg = 0; gg < G; ++gg) s += lds[gg * w + c];
        m.part[k][(long)blockIdx.x * w + c] = s;
    }
}

// STD false: mean = sum / length; true: std = sqrt(sum / length).  The partials of the workgroups that hold rows, thread t those
// t, t + 256, ... in that order, then a tree over the 256 threads: one order whatever the machine does.
template <bool STD>
__global__ void ds_final_kernel(const Moments m, long limit, const long *header) {
    __shared__ double lds[kThreads];
    const int k = blockIdx.y, w = m.w[k], c = blockIdx.x, t = threadIdx.x;
    if (c >= w) return;
    const long length = clampl(header[1], 0, limit);
    const long nblocks = (length + kMomentRows - 1) / kMomentRows;
    double s = 0.0;
    for (long i = t; i < nblocks; i += kThreads) s += m.part[k][i * w + c];
    lds[t] = s;
    __syncthreads();
    for (int d = kThreads / 2; d > 0; d >>= 1) {
        if (t < d) lds[t] += lds[t + d];
        __syncthreads();
    }
    if (t == 0) {
        const double q = lds[0] / (double)length;                       // 0 / 0 = NaN for an empty data set, as numpy
        if (STD) m.std[k][c] = sqrt(q);
        else m.mean[k][c] = q;
    }
}

// ---- batch ------------------------------------------------------------------------------------------------------------------------------

__global__ void ds_batch_kernel(const bmpc_dataset_t ds, const bmpc_dataset_batch_t q) {
    const int lane = threadIdx.x & (kWave - 1);
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
    if (i >= q.n) return;
    const long length = clampl(ds.header[1], 0, ds.limit);
    const long row = q.index[i];
    const bool in = row >= 0 && row < length;
    const bool cc = q.goal_type == BMPC_DS_GOAL_CC;
    const int ws = ds.w_states, wg = cc ? ds.w_cc : ds.w_vc, wa = ds.w_actions, wx = ws + wg;
    const double *goal = cc ? ds.cc_goals : ds.vc_goals;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int c = lane; c < wx + wa; c += kWave) {
        double v = nan;
        if (in) {
            if (c < ws) {
                v = ds.states[row * ws + c];
                if (q.normalise) v = (v - q.states_mean[c]) / q.states_std[c];
            } else if (c < wx) {
                const int cg = c - ws;
                v = goal[row * wg + cg];
                if (q.normalise) v = cc ? (v - q.goal_mean[cg]) / q.goal_std[cg] : (v - 0.0) / 1.0;
            } else {
                v = ds.actions[row * wa + (c - wx)];
            }
        }
        if (c < wx) q.x[i * wx + c] = v;
        else q.y[i * wa + (c - wx)] = v;
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------

int bad(const std::string &msg) { return set_error(BMPC_BAD_ARG, msg); }

bool cc_width_ok(int w) { return w >= 0 && w <= BMPC_DS_MAX_CC_WIDTH && w % 3 == 0; }

int check_dataset(const bmpc_dataset_t *ds) {
    if (!ds) return bad("null data set descriptor (bmpc_dataset_t)");
    if (ds->limit < 1 || ds->limit >= (1L << 31)) return bad("limit must be in [1, 2^31), got " + std::to_string(ds->limit));
    if (ds->w_states != BMPC_DS_STATE_WIDTH) return bad("w_states must be 43, got " + std::to_string(ds->w_states));
    if (ds->w_vc != BMPC_DS_VC_WIDTH) return bad("w_vc must be 5, got " + std::to_string(ds->w_vc));
    if (ds->w_actions != BMPC_DS_ACTION_WIDTH) return bad("w_actions must be 12, got " + std::to_string(ds->w_actions));
    if (!cc_width_ok(ds->w_cc)) return bad("w_cc must be 0 or a multiple of 3 up to 768, got " + std::to_string(ds->w_cc));
    if (ds->max_problems < 1 || ds->max_problems > BMPC_DS_MAX_PROBLEMS)
        return bad("max_problems must be in [1, 2^24], got " + std::to_string(ds->max_problems));
    if (!ds->states) return bad("null data set array: states");
    if (!ds->vc_goals) return bad("null data set array: vc_goals");
    if (ds->w_cc && !ds->cc_goals) return bad("null data set array: cc_goals (w_cc = " + std::to_string(ds->w_cc) + ")");
    if (!ds->actions) return bad("null data set array: actions");
    if (!ds->header) return bad("null data set header");
    if (!ds->scratch) return bad("null data set scratch");
    if (reinterpret_cast<uintptr_t>(ds->scratch) & 15) return bad("scratch must be 16-byte aligned");
    const long need = scratch_layout(ds->limit, ds->w_cc, ds->max_problems).bytes;
    if (ds->scratch_bytes < need)
        return bad("scratch_bytes must be bmpc_dataset_scratch_bytes(...) = " + std::to_string(need) + " at least, got " + std::to_string(ds->scratch_bytes));
    return BMPC_OK;
}

template <class T>
T *in_scratch(const bmpc_dataset_t *ds, long offset) { return reinterpret_cast<T *>(static_cast<char *>(ds->scratch) + offset); }

int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(BMPC_DEVICE_ERROR, std::string(what) + hipGetErrorString(e));
    return BMPC_OK;
}

}  // namespace
}  // namespace bunmpc

extern "C" int bmpc_dataset_struct_size(void) { return (int)sizeof(bmpc_dataset_t); }
extern "C" int bmpc_dataset_rows_struct_size(void) { return (int)sizeof(bmpc_dataset_rows_t); }
extern "C" int bmpc_dataset_batch_struct_size(void) { return (int)sizeof(bmpc_dataset_batch_t); }

extern "C" long bmpc_dataset_scratch_bytes(long limit, int w_cc, int max_problems) {
    using namespace bunmpc;
    if (limit < 1 || limit >= (1L << 31) || !cc_width_ok(w_cc) || max_problems < 1 || max_problems > BMPC_DS_MAX_PROBLEMS) return -1;
    return scratch_layout(limit, w_cc, max_problems).bytes;
}

extern "C" int bmpc_dataset_append_device(const bmpc_dataset_t *ds, const bmpc_dataset_rows_t *rows, void *hip_stream) {
    using namespace bunmpc;
    if (int rc = check_dataset(ds)) return rc;
    if (!rows) return bad("null rows descriptor (bmpc_dataset_rows_t)");
    if (rows->B < 0 || rows->B > ds->max_problems)
        return bad("B must be in [0, max_problems = " + std::to_string(ds->max_problems) + "], got " + std::to_string(rows->B));
    if (rows->R < 1) return bad("R must be >= 1, got " + std::to_string(rows->R));
    if ((long)rows->B * rows->R >= (1L << 31)) return bad("B R must be below 2^31, got " + std::to_string((long)rows->B * rows->R));
    if ((long)rows->R * BMPC_DS_MAX_CC_WIDTH >= (1L << 31)) return bad("R must be below 2^31 / 768, got " + std::to_string(rows->R));
    if (rows->cc_goals && ds->w_cc == 0) return bad("cc_goals given to a data set without that group (w_cc = 0)");
    if (rows->w_states != ds->w_states) return bad("rows w_states differs from the data set's: " + std::to_string(rows->w_states));
    if (rows->w_vc != ds->w_vc) return bad("rows w_vc differs from the data set's: " + std::to_string(rows->w_vc));
    if (rows->w_cc != ds->w_cc) return bad("rows w_cc differs from the data set's: " + std::to_string(rows->w_cc) + " against " + std::to_string(ds->w_cc));
    if (rows->w_actions != ds->w_actions) return bad("rows w_actions differs from the data set's: " + std::to_string(rows->w_actions));
    if (!rows->states) return bad("null rows array: states");
    if (!rows->actions) return bad("null rows array: actions");
    if (!rows->vc_goals && !rows->cc_goals) return bad("both vc_goals and cc_goals cant be empty!");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const Scratch s = scratch_layout(ds->limit, ds->w_cc, ds->max_problems);
    int *counts = in_scratch<int>(ds, s.counts);
    long *local = in_scratch<long>(ds, s.local), *chunk_tot = in_scratch<long>(ds, s.chunk_tot), *chunk_off = in_scratch<long>(ds, s.chunk_off);
    long *total = in_scratch<long>(ds, s.total);
    Groups g;
    const double *src[kGroups] = {rows->states, rows->actions, rows->vc_goals, rows->cc_goals};
    double *dst[kGroups] = {ds->states, ds->actions, ds->vc_goals, ds->cc_goals};
    const int w[kGroups] = {ds->w_states, ds->w_actions, ds->w_vc, ds->w_cc};
    int w_max = 0;
    for (int k = 0; k < kGroups; ++k) {
        g.src[k] = src[k];
        g.dst[k] = dst[k];
        g.w[k] = w[k];
        if (src[k] && w[k] > w_max) w_max = w[k];
    }
    const int B = rows->B, R = rows->R;
    const long nchunks = ((long)B + kChunk - 1) / kChunk;                 // <= s.nchunks: B <= max_problems
    const long pairs = (long)B * (((long)R * w_max + 1) / 2);
    if ((pairs + kThreads - 1) / kThreads >= (1L << 31)) return bad("B R times the widest group is more than one launch takes: B R = " + std::to_string((long)B * R));
    if (B > 0) {
        hipLaunchKernelGGL(ds_count_kernel, dim3((unsigned)(((long)B * kWave + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, g, B, R, rows->rows,
                           rows->keep, rows->drop_nonfinite, counts);
        hipLaunchKernelGGL(ds_chunk_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, st, B, R, counts, local, chunk_tot);
    }
    hipLaunchKernelGGL(ds_offsets_kernel, dim3(1), dim3(kThreads), 0, st, nchunks, chunk_tot, chunk_off, total);
    if (B > 0) {
        hipLaunchKernelGGL(ds_scatter_kernel, dim3((unsigned)((pairs + kThreads - 1) / kThreads), kGroups), dim3(kThreads), 0, st, g, B, R, ds->limit,
                           ds->header, counts, local, chunk_off, total);
    }
    hipLaunchKernelGGL(ds_header_kernel, dim3(1), dim3(1), 0, st, ds->limit, (long)B * R, total, ds->header);
    return launched("data set append kernels: ");
}

extern "C" int bmpc_dataset_moments_device(const bmpc_dataset_t *ds, double *states_mean, double *states_std, double *cc_mean, double *cc_std,
                                           void *hip_stream) {
    using namespace bunmpc;
    if (int rc = check_dataset(ds)) return rc;
    if (!states_mean) return bad("null output array: states_mean");
    if (!states_std) return bad("null output array: states_std");
    if (ds->w_cc && !cc_mean) return bad("null output array: cc_mean");
    if (ds->w_cc && !cc_std) return bad("null output array: cc_std");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const Scratch s = scratch_layout(ds->limit, ds->w_cc, ds->max_problems);
    Moments m;
    m.buf[0] = ds->states;  m.w[0] = ds->w_states;  m.part[0] = in_scratch<double>(ds, s.part_states);  m.mean[0] = states_mean;  m.std[0] = states_std;
    m.buf[1] = ds->cc_goals;  m.w[1] = ds->w_cc;  m.part[1] = in_scratch<double>(ds, s.part_cc);  m.mean[1] = cc_mean;  m.std[1] = cc_std;
    const dim3 partial((unsigned)s.nblocks, 2), final_((unsigned)(ds->w_cc > ds->w_states ? ds->w_cc : ds->w_states), 2);
    hipLaunchKernelGGL(ds_partial_kernel<false>, partial, dim3(kThreads), 0, st, m, ds->limit, ds->header);
    hipLaunchKernelGGL(ds_final_kernel<false>, final_, dim3(kThreads), 0, st, m, ds->limit, ds->header);
    hipLaunchKernelGGL(ds_partial_kernel<true>, partial, dim3(kThreads), 0, st, m, ds->limit, ds->header);
    hipLaunchKernelGGL(ds_final_kernel<true>, final_, dim3(kThreads), 0, st, m, ds->limit, ds->header);
    return launched("data set moment kernels: ");
}

extern "C" int bmpc_dataset_batch_device(const bmpc_dataset_t *ds, const bmpc_dataset_batch_t *batch, void *hip_stream) {
    using namespace bunmpc;
    if (int rc = check_dataset(ds)) return rc;
    if (!batch) return bad("null batch descriptor (bmpc_dataset_batch_t)");
    if (batch->n < 0 || batch->n >= (1L << 31)) return bad("n must be in [0, 2^31), got " + std::to_string(batch->n));
    if (batch->goal_type != BMPC_DS_GOAL_VC && batch->goal_type != BMPC_DS_GOAL_CC)
        return bad("goal_type must be BMPC_DS_GOAL_VC or BMPC_DS_GOAL_CC, got " + std::to_string(batch->goal_type));
    if (batch->goal_type == BMPC_DS_GOAL_CC && ds->w_cc == 0) return bad("goal_type cc asked of a data set without that group (w_cc = 0)");
    if (!batch->index) return bad("null batch array: index");
    if (!batch->x) return bad("null batch array: x");
    if (!batch->y) return bad("null batch array: y");
    if (batch->normalise) {
        if (!batch->states_mean) return bad("null batch array: states_mean (normalise is set)");
        if (!batch->states_std) return bad("null batch array: states_std (normalise is set)");
        if (batch->goal_type == BMPC_DS_GOAL_CC && !batch->goal_mean) return bad("null batch array: goal_mean (normalise is set, goal_type cc)");
        if (batch->goal_type == BMPC_DS_GOAL_CC && !batch->goal_std) return bad("null batch array: goal_std (normalise is set, goal_type cc)");
    }
    if (batch->n == 0) return BMPC_OK;
    const long blocks = (batch->n * kWave + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(ds_batch_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, static_cast<hipStream_t>(hip_stream), *ds, *batch);
    return launched("data set batch kernel: ");
}
