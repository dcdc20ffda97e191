// The policy network's forward pass (include/ext/bunmpc_policy.h): GoalConditionedPolicyNet of ISL/examples/iterative_algorithm/networks.py
// in eval() mode, one launch per call.  bunmpc_amd/policy.py::host_forward is the numpy restatement the tests compare with, bit for bit.
//
//   workgroup   kTile = 32 rows, 4 waves; the activations of its rows stay in LDS as fp32 in two buffers that the layers alternate between
//   prologue    the rows' fp64 input (x, or state | goal normalised), rounded to fp32, into the first buffer; rows past n and columns past
//               n_in are +0
//   layer       wave w takes the 16-column output tiles jt = w, w + 4, ...; per tile two accumulators (rows 0-15, 16-31) start as the bias and
//               run v_mfma_f32_16x16x4_f32 over k ascending: A = the activations (row r = lane % 16, k = 4 step + lane / 16) from LDS,
//               B = the weights (column j = lane % 16, same k) from the packed image, 16 bytes per lane per four steps; D has column j on
//               lane % 16 and rows 4 (lane / 16) + reg, so bias, BatchNorm and ReLU are per-lane and a lane stores four consecutive rows
//   epilogue    action, tau, err from the last layer's LDS image
// LDS image: act[k][32] with the row index XORed by 16 where k is odd -- the two k of a wave's 32-lane half then read banks 0-15 and
// 16-31 (ds_read_b32 banks are dword % 32), and a lane's four rows stay 16 contiguous bytes.
// Every global address is bounded by what the host checked: rows by n, columns by the widths, the packed image by packed_bytes.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/bunmpc.h"
#include "../../include/ext/bunmpc_policy.h"

// the normalisation, tau and err are held to numpy's operations one by one, and the host packer to its twin: no fused multiply-add but fmaf
#pragma clang fp contract(off)

namespace bunmpc {
int set_error(int code, const std::string &msg);
namespace {

constexpr int kTile = 32, kThreads = 256, kWave = 64, kWaves = kThreads / kWave, kPad = BMPC_POLICY_PAD;
static_assert(kPad == 16, "a packed tile is 16 columns by 16 k");

typedef float f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int pad16(int v) { return (v + kPad - 1) / kPad * kPad; }

// floats of layer l's block of the packed image: W [Np][Kp], b [Np], and s, t [Np] with BatchNorm on a hidden layer
__host__ __device__ inline long layer_floats(int K, int N, bool bn) { return (long)pad16(N) * pad16(K) + (long)pad16(N) * (bn ? 3 : 1); }

long packed_floats(int n_in, int n_hidden, int n_layers, int n_out, int batch_norm) {
    long total = 0;
    for (int l = 0; l <= n_layers; ++l)
        total += layer_floats(l == 0 ? n_in : n_hidden, l == n_layers ? n_out : n_hidden, batch_norm && l < n_layers);
    return total;
}

int widest(int n_in, int n_hidden, int n_out) {
    const int a = pad16(n_in), b = pad16(n_hidden), c = pad16(n_out);
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

__device__ __forceinline__ int lds_at(int k, int r) { return k * kTile + (r ^ ((k & 1) << 4)); }

__global__ __launch_bounds__(kThreads) void policy_forward_kernel(const bmpc_policy_net_t net, const bmpc_policy_rows_t q, int wmax) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *cur = lds, *nxt = lds + wmax * kTile;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long r0 = (long)blockIdx.x * kTile;
    const int n_in = net.n_in, n_out = net.n_out;

    // ---- prologue: thread e takes column e % Kp of row e / Kp, so a wave reads along a row -------------------------------------------
    {
        const int Kp = pad16(n_in);
        for (int e = tid; e < kTile * Kp; e += kThreads) {
            const int r = e / Kp, k = e - r * Kp;
            const long row = r0 + r;
            float f = 0.0f;
            if (k < n_in && row < q.n) {
                double v;
                if (q.x) v = q.x[row * q.x_stride + k];
                else if (k < BMPC_POLICY_STATE_WIDTH) v = q.state[row * q.state_stride + k];
                else v = q.goal[row * q.goal_stride + (k - BMPC_POLICY_STATE_WIDTH)];
                if (q.mean) v = (v - q.mean[k]) / q.std[k];
                f = (float)v;
            }
            cur[lds_at(k, r)] = f;
        }
    }
    __syncthreads();

    // ---- the layers ------------------------------------------------------------------------------------------------------------------------
    const int c = lane & 15, g = lane >> 4;
    const int a0 = g * kTile + (c ^ ((g & 1) << 4)), a1 = a0 ^ 16;                    // lds_at(g, c), lds_at(g, c + 16)
    const float *p = static_cast<const float *>(net.packed);
    for (int l = 0; l <= net.n_layers; ++l) {
        const bool hidden = l < net.n_layers, bn = hidden && net.batch_norm;
        const int K = l == 0 ? n_in : net.n_hidden, N = hidden ? net.n_hidden : n_out;
        const int Kp = pad16(K), Np = pad16(N);
        const float *W = p, *b = W + (long)Np * Kp, *s = b + Np, *t = s + Np;
        p += layer_floats(K, N, bn);
        for (int jt = wave; jt < Np / 16; jt += kWaves) {                           // (the same for a whole wave: every MFMA runs with all lanes)
            const int j = 16 * jt + c;
            const float bias = b[j];
            f32x4 acc0 = {bias, bias, bias, bias}, acc1 = acc0;
            const f32x4 *wp = reinterpret_cast<const f32x4 *>(W + (long)jt * Kp * 16) + lane;
            const float *ap = cur;
            for (int kq = 0; kq < Kp / 16; ++kq, ap += 16 * kTile) {
                const f32x4 w = wp[kq * kWave];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[a0 + 4 * i * kTile], w[i], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[a1 + 4 * i * kTile], w[i], acc1, 0, 0, 0);
                }
            }
            if (bn) {
                const float sj = s[j], tj = t[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc0[i] = fmaf(acc0[i], sj, tj);
                    acc1[i] = fmaf(acc1[i], sj, tj);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (hidden) {
                    acc0[i] = acc0[i] <= 0.0f ? 0.0f : acc0[i];
                    acc1[i] = acc1[i] <= 0.0f ? 0.0f : acc1[i];
                }
                if (j >= N) acc0[i] = acc1[i] = 0.0f;                               // the next layer's padding is +0 whatever the row holds
            }
            const int at = j * kTile + ((4 * g) ^ ((j & 1) << 4));                   // lds_at(j, 4 g): rows 4 g .. 4 g + 3 follow
            *reinterpret_cast<f32x4 *>(nxt + at) = acc0;
            *reinterpret_cast<f32x4 *>(nxt + (at ^ 16)) = acc1;
        }
        __syncthreads();
        float *swap = cur;
        cur = nxt;
        nxt = swap;
    }

    // ---- epilogue: cur holds the output layer, column j of row r at lds_at(j, r) -------------------------------------------------------
    if (q.action) {
        for (int e = tid; e < kTile * n_out; e += kThreads) {
            const int r = e / n_out, j = e - r * n_out;
            if (r0 + r < q.n) q.action[(r0 + r) * n_out + j] = (double)cur[lds_at(j, r)];
        }
    }
    if (q.tau) {
        for (int e = tid; e < kTile * BMPC_POLICY_TAU_WIDTH; e += kThreads) {
            const int r = e / BMPC_POLICY_TAU_WIDTH, i = e - r * BMPC_POLICY_TAU_WIDTH;
            const long row = r0 + r;
            if (row >= q.n) continue;
            const double a = (double)cur[lds_at(i, r)];
            double tau = a;
            if (q.action_type != BMPC_POLICY_TORQUE) {
                const double qi = q.q[row * q.q_stride + 7 + i], vi = q.v[row * q.v_stride + 6 + i];
                if (q.action_type == BMPC_POLICY_PD_TARGET) {
                    tau = q.kp * (a - qi) - q.kd * vi;
                } else {
                    const double q_des = (double)cur[lds_at(12 + i, r)], dq_des = (double)cur[lds_at(24 + i, r)];
                    tau = (a + q.kp * (q_des - qi)) + q.kd * (dq_des - vi);
                }
            }
            q.tau[row * BMPC_POLICY_TAU_WIDTH + i] = tau;
        }
    }
    if (q.err && tid < kTile && r0 + tid < q.n) {
        const double *label = q.label + (r0 + tid) * q.label_stride;
        double e = 0.0;
        for (int j = 0; j < n_out; ++j) e = e + fabs((double)cur[lds_at(j, tid)] - (double)(float)label[j]);
        q.err[r0 + tid] = e;
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------

int bad(const std::string &msg) { return set_error(BMPC_BAD_ARG, msg); }

int check_net(const bmpc_policy_net_t *net) {
    if (!net) return bad("null network descriptor (bmpc_policy_net_t)");
    if (net->n_in < 1 || net->n_in > BMPC_POLICY_MAX_WIDTH) return bad("n_in must be in [1, 512], got " + std::to_string(net->n_in));
    if (net->n_hidden < 1 || net->n_hidden > BMPC_POLICY_MAX_WIDTH) return bad("n_hidden must be in [1, 512], got " + std::to_string(net->n_hidden));
    if (net->n_layers < 1 || net->n_layers > BMPC_POLICY_MAX_LAYERS) return bad("n_layers must be in [1, 8], got " + std::to_string(net->n_layers));
    if (net->n_out < 1 || net->n_out > BMPC_POLICY_MAX_OUT) return bad("n_out must be in [1, 64], got " + std::to_string(net->n_out));
    const long need = 4 * packed_floats(net->n_in, net->n_hidden, net->n_layers, net->n_out, net->batch_norm);
    if (net->packed_bytes != need)
        return bad("packed_bytes must be bmpc_policy_packed_bytes(...) = " + std::to_string(need) + ", got " + std::to_string(net->packed_bytes));
    if (!net->packed) return bad("null packed image: packed");
    if (reinterpret_cast<uintptr_t>(net->packed) & 15) return bad("packed must be 16-byte aligned");
    return BMPC_OK;
}

}  // namespace
}  // namespace bunmpc

extern "C" int bmpc_policy_net_struct_size(void) { return (int)sizeof(bmpc_policy_net_t); }
extern "C" int bmpc_policy_weights_struct_size(void) { return (int)sizeof(bmpc_policy_weights_t); }
extern "C" int bmpc_policy_rows_struct_size(void) { return (int)sizeof(bmpc_policy_rows_t); }
extern "C" int bmpc_policy_tile(void) { return bunmpc::kTile; }

extern "C" long bmpc_policy_packed_bytes(int n_in, int n_hidden, int n_layers, int n_out, int batch_norm) {
    if (n_in < 1 || n_in > BMPC_POLICY_MAX_WIDTH || n_hidden < 1 || n_hidden > BMPC_POLICY_MAX_WIDTH || n_layers < 1 ||
        n_layers > BMPC_POLICY_MAX_LAYERS || n_out < 1 || n_out > BMPC_POLICY_MAX_OUT)
        return -1;
    return 4 * bunmpc::packed_floats(n_in, n_hidden, n_layers, n_out, batch_norm);
}

extern "C" int bmpc_policy_pack_host(const bmpc_policy_net_t *net, const bmpc_policy_weights_t *weights) {
    using namespace bunmpc;
    if (int rc = check_net(net)) return rc;
    if (!weights) return bad("null weights descriptor (bmpc_policy_weights_t)");
    for (int l = 0; l <= net->n_layers; ++l) {
        if (!weights->W[l]) return bad("null weight array: W[" + std::to_string(l) + "]");
        if (!weights->b[l]) return bad("null weight array: b[" + std::to_string(l) + "]");
        if (net->batch_norm && l < net->n_layers) {
            if (!weights->gamma[l]) return bad("null weight array: gamma[" + std::to_string(l) + "]");
            if (!weights->beta[l]) return bad("null weight array: beta[" + std::to_string(l) + "]");
            if (!weights->running_mean[l]) return bad("null weight array: running_mean[" + std::to_string(l) + "]");
            if (!weights->running_var[l]) return bad("null weight array: running_var[" + std::to_string(l) + "]");
        }
    }
    float *p = static_cast<float *>(const_cast<void *>(net->packed));
    std::memset(p, 0, (size_t)net->packed_bytes);
    for (int l = 0; l <= net->n_layers; ++l) {
        const bool bn = net->batch_norm && l < net->n_layers;
        const int K = l == 0 ? net->n_in : net->n_hidden, N = l == net->n_layers ? net->n_out : net->n_hidden;
        const int Kp = pad16(K), Np = pad16(N);
        const float *W = static_cast<const float *>(weights->W[l]), *b = static_cast<const float *>(weights->b[l]);
        for (int j = 0; j < N; ++j) {
            for (int k = 0; k < K; ++k) {
                const int jt = j / 16, kq = k / 16, i = (k % 16) / 4, lane = 16 * (k % 4) + j % 16;
                p[(((long)jt * (Kp / 16) + kq) * kWave + lane) * 4 + i] = W[(long)j * K + k];
            }
        }
        float *pb = p + (long)Np * Kp;
        for (int j = 0; j < N; ++j) pb[j] = b[j];
        if (bn) {
            const float *gamma = static_cast<const float *>(weights->gamma[l]), *beta = static_cast<const float *>(weights->beta[l]);
            const float *mean = static_cast<const float *>(weights->running_mean[l]), *var = static_cast<const float *>(weights->running_var[l]);
            for (int j = 0; j < N; ++j) {
                const double s = (double)gamma[j] / std::sqrt((double)var[j] + weights->eps);
                const double t = (double)beta[j] - (double)mean[j] * s;
                pb[Np + j] = (float)s;
                pb[2 * Np + j] = (float)t;
            }
        }
        p += layer_floats(K, N, bn);
    }
    return BMPC_OK;
}

extern "C" int bmpc_policy_forward_device(const bmpc_policy_net_t *net, const bmpc_policy_rows_t *rows, void *hip_stream) {
    using namespace bunmpc;
    if (int rc = check_net(net)) return rc;
    if (!rows) return bad("null rows descriptor (bmpc_policy_rows_t)");
    if (rows->n < 0 || rows->n >= (1L << 31)) return bad("n must be in [0, 2^31), got " + std::to_string(rows->n));
    if (rows->x) {
        if (rows->state || rows->goal) return bad("both input forms given: x beside state / goal");
        if (rows->x_stride < net->n_in) return bad("x_stride must be n_in = " + std::to_string(net->n_in) + " at least, got " + std::to_string(rows->x_stride));
        if (rows->mean || rows->std) return bad("mean / std go with the state, goal form, not with x");
    } else {
        if (!rows->state && !rows->goal) return bad("no input: neither x nor state, goal");
        if (!rows->state) return bad("null input array: state");
        if (!rows->goal) return bad("null input array: goal");
        const int w_goal = net->n_in - BMPC_POLICY_STATE_WIDTH;
        if (w_goal < 1) return bad("state, goal need n_in = 43 + w_goal with w_goal >= 1, got n_in = " + std::to_string(net->n_in));
        if (rows->state_stride < BMPC_POLICY_STATE_WIDTH) return bad("state_stride must be 43 at least, got " + std::to_string(rows->state_stride));
        if (rows->goal_stride < w_goal) return bad("goal_stride must be n_in - 43 = " + std::to_string(w_goal) + " at least, got " + std::to_string(rows->goal_stride));
        if (!rows->mean != !rows->std) return bad(std::string("mean and std go together: null ") + (rows->mean ? "std" : "mean"));
    }
    if (rows->tau) {
        const int t = rows->action_type;
        if (t != BMPC_POLICY_TORQUE && t != BMPC_POLICY_PD_TARGET && t != BMPC_POLICY_STRUCTURED)
            return bad("action_type must be BMPC_POLICY_TORQUE, _PD_TARGET or _STRUCTURED, got " + std::to_string(t));
        const int want = t == BMPC_POLICY_STRUCTURED ? 3 * BMPC_POLICY_TAU_WIDTH : BMPC_POLICY_TAU_WIDTH;
        if (net->n_out != want) return bad("tau of action_type " + std::to_string(t) + " needs n_out = " + std::to_string(want) + ", got " + std::to_string(net->n_out));
        if (t != BMPC_POLICY_TORQUE) {
            if (!rows->q) return bad("null array: q (tau is asked for)");
            if (!rows->v) return bad("null array: v (tau is asked for)");
            if (rows->q_stride < BMPC_POLICY_Q_WIDTH) return bad("q_stride must be 19 at least, got " + std::to_string(rows->q_stride));
            if (rows->v_stride < BMPC_POLICY_V_WIDTH) return bad("v_stride must be 18 at least, got " + std::to_string(rows->v_stride));
        }
    }
    if (rows->err) {
        if (!rows->label) return bad("null array: label (err is asked for)");
        if (rows->label_stride < net->n_out) return bad("label_stride must be n_out = " + std::to_string(net->n_out) + " at least, got " + std::to_string(rows->label_stride));
    }
    if (rows->n == 0) return BMPC_OK;
    const int wmax = widest(net->n_in, net->n_hidden, net->n_out);
    const size_t lds_bytes = 2 * (size_t)wmax * kTile * sizeof(float);      // 128 KiB at the widest
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(policy_forward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return set_error(BMPC_DEVICE_ERROR, std::string("policy forward kernel, LDS of ") + std::to_string(lds_bytes) + " bytes: " + hipGetErrorString(e));
    }
    const long blocks = (rows->n + kTile - 1) / kTile;
    hipLaunchKernelGGL(policy_forward_kernel, dim3((unsigned)blocks), dim3(kThreads), lds_bytes, static_cast<hipStream_t>(hip_stream), *net, *rows, wmax);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(BMPC_DEVICE_ERROR, std::string("policy forward kernel: ") + hipGetErrorString(e));
    return BMPC_OK;
}
