// The policy network's training step (include/ext/bunmpc_policy_train.h): GoalConditionedPolicyNet in train() mode, nn.L1Loss, backward and
// Adam, and the packed inference image written on the device.  bunmpc_amd/policy_train.py::host_step is the numpy restatement the tests
// compare with, bit for bit.
//
// Every reduction of the header is one ascending fmaf chain owned by one lane, so no result depends on the launch geometry:
//   input     x (fp64, strided) rounded to fp32 and transposed: every activation and gradient between the kernels is held column-major,
//             [column][n], so that a wave of consecutive rows reads and writes consecutive addresses
//   forward   per layer: a workgroup owns kCols output columns for ALL rows; thread r runs the k-ascending chains of its rows (the weights
//             are wave-uniform), and with BatchNorm the columns' values stay in LDS while one lane per column runs the two row-ascending
//             chains of the statistics, updates the running statistics, and the workgroup then normalises
//   loss      one workgroup: thread r sums its row in fp64 and writes dz of the output layer, lane 0 sums the rows ascending
//   da        per layer l >= 1: a workgroup owns kCols columns k of the layer below for all rows; thread r runs the j-ascending chain
//             W[j][k] dz[r][j], applies the ReLU mask, and with BatchNorm one lane per column chains dbeta and dgamma over the rows in
//             LDS, takes that column's Adam step on gamma and beta, and the workgroup forms dz of the layer below
//   dW        per layer: a workgroup owns a 16 x 16 tile of dW (and db beside its first column of tiles); dz and the activations pass
//             through LDS in chunks of kChunk rows, each thread chains its element over the rows ascending and takes its Adam step
// da of layer l reads W[l] and runs before dW of layer l rewrites it; the order on the stream is the only synchronisation.
// Every global address is bounded by what the host checked: rows by n, columns by the widths, the scratch by work_bytes.
#include <cmath>
#include <cstdint>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/bunmpc.h"
#include "../../include/ext/bunmpc_policy.h"
#include "../../include/ext/bunmpc_policy_train.h"

// every operation is held to numpy's one by one: no fused multiply-add but fmaf
#pragma clang fp contract(off)

namespace bunmpc {
int set_error(int code, const std::string &msg);
namespace {

constexpr int kThreads = 256, kCols = 4, kMaxRows = BMPC_POLICY_TRAIN_MAX_ROWS, kPad = BMPC_POLICY_TRAIN_PAD, kChunk = 64, kWave = 64;
static_assert(kPad == BMPC_POLICY_PAD, "one padding for the forward pass and the training step");
static_assert(kMaxRows % kThreads == 0 && kMaxRows % kChunk == 0, "row passes");

__host__ __device__ constexpr int pad16(int v) { return (v + kPad - 1) / kPad * kPad; }
__host__ __device__ inline long layer_floats(int K, int N, bool bn) { return (long)pad16(N) * pad16(K) + (long)pad16(N) * (bn ? 3 : 1); }

// IEEE fp32 sqrt and divide: the fp64 operation rounded once more (53 >= 2 * 24 + 2 bits: the second rounding changes nothing)
__device__ __forceinline__ float sqrt32(float a) { return (float)sqrt((double)a); }
__device__ __forceinline__ float div32(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float relu(float u) { return u <= 0.0f ? 0.0f : u; }

struct Adam {
    float w1, w2, b2, step, root, eps;
};

// step g on one element
__device__ __forceinline__ void adam_step(const Adam &k, float g, float *q, float *m, float *v) {
    const float m1 = fmaf(k.w1, g - *m, *m);
    const float v1 = fmaf(k.w2 * g, g, k.b2 * *v);
    const float denom = div32(sqrt32(v1), k.root) + k.eps;
    *q = fmaf(-k.step, div32(m1, denom), *q);
    *m = m1;
    *v = v1;
}

// ---- step a: x [n][n_in] fp64 -> a_0 [n_in][n] fp32 ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void train_input_kernel(const double *x, long x_stride, int n, int n_in, float *aT) {
    const long e = (long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (long)n * n_in) return;
    const int r = (int)(e / n_in), k = (int)(e - (long)r * n_in);
    aT[(long)k * n + r] = (float)x[r * x_stride + k];
}

// ---- steps b to d for one layer ----------------------------------------------------------------------------------------------------------
struct Forward {
    const float *W, *b, *aT;          // [N][K], [N], [K][n]
    float *outT;                      // [N][n]: the next layer's activations, or the prediction
    float *xhatT, *invstd;            // [N][n], [N]  (BatchNorm)
    const float *gamma, *beta;
    float *running_mean, *running_var;
    int K, N, n, bn, last;
    float eps;
};

__global__ __launch_bounds__(kThreads) void train_forward_kernel(const Forward f) {
    __shared__ float zs[kCols][kMaxRows];
    __shared__ float mean_s[kCols], invstd_s[kCols];
    const int tid = threadIdx.x, j0 = blockIdx.x * kCols, n = f.n, K = f.K;
    const float *w[kCols];
    float bias[kCols];
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
        const int j = j0 + c < f.N ? j0 + c : f.N - 1;      // a column past N repeats the last one and is not stored
        w[c] = f.W + (long)j * K;
        bias[c] = f.b[j];
    }
    for (int r = tid; r < n; r += kThreads) {
        float acc[kCols];
#pragma unroll
        for (int c = 0; c < kCols; ++c) acc[c] = bias[c];
        const float *a = f.aT + r;
#pragma unroll 8
        for (int k = 0; k < K; ++k) {
            const float ak = a[(long)k * n];
#pragma unroll
            for (int c = 0; c < kCols; ++c) acc[c] = fmaf(w[c][k], ak, acc[c]);
        }
        if (K % kPad) {
#pragma unroll
            for (int c = 0; c < kCols; ++c) acc[c] = fmaf(0.0f, 0.0f, acc[c]);
        }
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
            if (f.bn) zs[c][r] = acc[c];
            else if (j0 + c < f.N) f.outT[(long)(j0 + c) * n + r] = f.last ? acc[c] : relu(acc[c]);
        }
    }
    if (!f.bn) return;
    __syncthreads();
    if (tid < kCols && j0 + tid < f.N) {      // one lane per column: the two chains over the rows, ascending
        const int j = j0 + tid;
        const float fn = (float)n;
        float s = 0.0f;
        for (int r = 0; r < n; ++r) s = fmaf(zs[tid][r], 1.0f, s);
        const float mean = div32(s, fn);
        float sq = 0.0f;
        for (int r = 0; r < n; ++r) {
            const float d = zs[tid][r] - mean;
            sq = fmaf(d, d, sq);
        }
        const float var = div32(sq, fn);
        const float invstd = div32(1.0f, sqrt32(var + f.eps));
        mean_s[tid] = mean;
        invstd_s[tid] = invstd;
        f.invstd[j] = invstd;
        const float mom = 0.1f, keep = 1.0f - mom;
        f.running_mean[j] = fmaf(mom, mean, keep * f.running_mean[j]);
        f.running_var[j] = fmaf(mom, div32(var * fn, fn - 1.0f), keep * f.running_var[j]);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
        const int j = j0 + c;
        if (j >= f.N) break;
        const float mean = mean_s[c], invstd = invstd_s[c], gamma = f.gamma[j], beta = f.beta[j];
        for (int r = tid; r < n; r += kThreads) {
            const float xh = (zs[c][r] - mean) * invstd;
            f.xhatT[(long)j * n + r] = xh;
            f.outT[(long)j * n + r] = relu(fmaf(xh, gamma, beta));
        }
    }
}

// ---- step e and the output layer's dz -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void train_loss_kernel(const float *pT, const double *y, long y_stride, int n, int n_out, float *dzT, double *loss) {
    __shared__ double es[kMaxRows];
    const int tid = threadIdx.x;
    const float c = div32(1.0f, (float)(n * n_out));
    for (int r = tid; r < n; r += kThreads) {
        double e = 0.0;
        for (int j = 0; j < n_out; ++j) {
            const float p = pT[(long)j * n + r], y32 = (float)y[r * y_stride + j];
            e = e + fabs((double)p - (double)y32);
            const float t = p - y32;
            dzT[(long)j * n + r] = t > 0.0f ? c : t < 0.0f ? -c : t == 0.0f ? 0.0f : t;
        }
        es[r] = e;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int r = 0; r < n; ++r) s = s + es[r];
        *loss = s / (double)(n * n_out);
    }
}

// ---- step f, towards the layer below: da, the ReLU mask, BatchNorm's backward and its Adam step --------------------------------------------
struct Below {
    const float *W, *dzT;             // layer l: [N][K], [N][n]
    const float *aT;                  // a_l [K][n]: the mask
    const float *xhatT, *invstd;      // of layer l - 1: [K][n], [K]  (BatchNorm)
    float *gamma, *beta, *m_gamma, *m_beta, *v_gamma, *v_beta, *g_gamma, *g_beta;      // of layer l - 1; g_*: NULL or where the gradients go
    float *outT;                      // dz_{l-1} [K][n]
    int K, N, n, bn;
    Adam adam;
};

__global__ __launch_bounds__(kThreads) void train_below_kernel(const Below f) {
    __shared__ float du_s[kCols][kMaxRows], xh_s[kCols][kMaxRows];
    __shared__ float g_s[kCols], mb_s[kCols], mg_s[kCols];
    const int tid = threadIdx.x, k0 = blockIdx.x * kCols, n = f.n, K = f.K, N = f.N;
    int col[kCols];
#pragma unroll
    for (int c = 0; c < kCols; ++c) col[c] = k0 + c < K ? k0 + c : K - 1;      // a column past K repeats the last one and is not stored
    for (int r = tid; r < n; r += kThreads) {
        float acc[kCols];
#pragma unroll
        for (int c = 0; c < kCols; ++c) acc[c] = 0.0f;
        const float *dz = f.dzT + r;
#pragma unroll 8
        for (int j = 0; j < N; ++j) {
            const float d = dz[(long)j * n];
            const float *wj = f.W + (long)j * K;
#pragma unroll
            for (int c = 0; c < kCols; ++c) acc[c] = fmaf(wj[col[c]], d, acc[c]);
        }
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
            const long at = (long)col[c] * n + r;
            const float du = f.aT[at] <= 0.0f ? 0.0f : acc[c];
            if (f.bn) {
                du_s[c][r] = du;
                xh_s[c][r] = f.xhatT[at];
            } else if (k0 + c < K) {
                f.outT[at] = du;
            }
        }
    }
    if (!f.bn) return;
    __syncthreads();
    if (tid < kCols && k0 + tid < K) {      // one lane per column: dbeta and dgamma over the rows, ascending
        const int k = k0 + tid;
        const float fn = (float)n;
        float dbeta = 0.0f, dgamma = 0.0f;
        for (int r = 0; r < n; ++r) {
            dbeta = fmaf(du_s[tid][r], 1.0f, dbeta);
            dgamma = fmaf(du_s[tid][r], xh_s[tid][r], dgamma);
        }
        g_s[tid] = f.gamma[k] * f.invstd[k];
        mb_s[tid] = div32(dbeta, fn);
        mg_s[tid] = div32(dgamma, fn);
        if (f.g_gamma) {
            f.g_gamma[k] = dgamma;
            f.g_beta[k] = dbeta;
        }
        adam_step(f.adam, dgamma, f.gamma + k, f.m_gamma + k, f.v_gamma + k);
        adam_step(f.adam, dbeta, f.beta + k, f.m_beta + k, f.v_beta + k);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
        const int k = k0 + c;
        if (k >= K) break;
        const float g = g_s[c], mb = mb_s[c], mg = mg_s[c];
        for (int r = tid; r < n; r += kThreads) f.outT[(long)k * n + r] = fmaf(-xh_s[c][r], mg, du_s[c][r] - mb) * g;
    }
}

// ---- step f's dW and db with their Adam step ----------------------------------------------------------------------------------------------
struct Weights {
    const float *dzT, *aT;            // [N][n], [K][n]
    float *W, *b, *m_W, *m_b, *v_W, *v_b, *g_W, *g_b;      // g_*: NULL or where the gradients go
    int K, N, n;
    Adam adam;
};

__global__ __launch_bounds__(kThreads) void train_weights_kernel(const Weights f) {
    __shared__ float dz_s[16][kChunk + 1], a_s[16][kChunk + 1];
    const int tid = threadIdx.x, jj = tid >> 4, kk = tid & 15, j0 = blockIdx.y * 16, k0 = blockIdx.x * 16, n = f.n;
    const bool bias = blockIdx.x == 0 && kk == 0;
    float s = 0.0f, sb = 0.0f;
    for (int r0 = 0; r0 < n; r0 += kChunk) {
        __syncthreads();
        for (int e = tid; e < 16 * kChunk; e += kThreads) {
            const int c = e / kChunk, rr = e - c * kChunk, r = r0 + rr;      // rows past n and columns past the widths are +0 terms
            dz_s[c][rr] = r < n && j0 + c < f.N ? f.dzT[(long)(j0 + c) * n + r] : 0.0f;
            a_s[c][rr] = r < n && k0 + c < f.K ? f.aT[(long)(k0 + c) * n + r] : 0.0f;
        }
        __syncthreads();
        const int rows = n - r0 < kChunk ? n - r0 : kChunk;
        for (int rr = 0; rr < rows; ++rr) {
            const float d = dz_s[jj][rr];
            s = fmaf(d, a_s[kk][rr], s);
            if (bias) sb = fmaf(d, 1.0f, sb);
        }
    }
    const int j = j0 + jj, k = k0 + kk;
    if (j >= f.N) return;
    if (k < f.K) {
        const long at = (long)j * f.K + k;
        if (f.g_W) f.g_W[at] = s;
        adam_step(f.adam, s, f.W + at, f.m_W + at, f.v_W + at);
    }
    if (bias) {
        if (f.g_b) f.g_b[j] = sb;
        adam_step(f.adam, sb, f.b + j, f.m_b + j, f.v_b + j);
    }
}

// ---- the packed image of bmpc_policy_pack_host ----------------------------------------------------------------------------------------------
struct Pack {
    const float *W[9], *b[9], *gamma[8], *beta[8], *running_mean[8], *running_var[8];
    long at[9];                       // layer l's block of the image, in floats
    int n_in, n_hidden, n_layers, n_out, batch_norm;
    double eps;
    float *image;
};

__global__ __launch_bounds__(kThreads) void policy_pack_kernel(const Pack f) {
    const int l = blockIdx.y;
    const bool bn = f.batch_norm && l < f.n_layers;
    const int K = l == 0 ? f.n_in : f.n_hidden, N = l == f.n_layers ? f.n_out : f.n_hidden;
    const int Kp = pad16(K), Np = pad16(N);
    const long e = (long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= layer_floats(K, N, bn)) return;
    float *out = f.image + f.at[l];
    float value = 0.0f;
    if (e < (long)Np * Kp) {      // (jt, kq, lane, i) is W[16 jt + lane % 16][16 kq + 4 i + lane / 16]
        const int i = (int)(e & 3), lane = (int)((e >> 2) & (kWave - 1));
        const long tile = e >> 8;
        const int kq = (int)(tile % (Kp / 16)), jt = (int)(tile / (Kp / 16));
        const int j = 16 * jt + (lane & 15), k = 16 * kq + 4 * i + (lane >> 4);
        if (j < N && k < K) value = f.W[l][(long)j * K + k];
    } else {
        const long rest = e - (long)Np * Kp;
        const int which = (int)(rest / Np), j = (int)(rest - (long)which * Np);
        if (j < N) {
            if (which == 0) {
                value = f.b[l][j];
            } else {
                const double s = (double)f.gamma[l][j] / sqrt((double)f.running_var[l][j] + f.eps);
                value = which == 1 ? (float)s : (float)((double)f.beta[l][j] - (double)f.running_mean[l][j] * s);
            }
        }
    }
    out[e] = value;
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------

int bad(const std::string &msg) { return set_error(BMPC_BAD_ARG, msg); }

bool sizes_ok(int n_in, int n_hidden, int n_layers, int n_out) {
    return n_in >= 1 && n_in <= BMPC_POLICY_MAX_WIDTH && n_hidden >= 1 && n_hidden <= BMPC_POLICY_MAX_WIDTH && n_layers >= 1 &&
           n_layers <= BMPC_POLICY_MAX_LAYERS && n_out >= 1 && n_out <= BMPC_POLICY_MAX_OUT;
}

long round4(long v) { return (v + 3) / 4 * 4; }

// the scratch of a step of n rows, in floats: a_l [K_l][n] for l = 0 .. L, the prediction [n_out][n], two dz buffers [widest][n], and
// with BatchNorm xhat [H][n] and invstd [H] per hidden layer; every block starts at a multiple of 16 bytes
struct Work {
    long a[9], p, dz[2], xhat[8], invstd[8], total;
};

Work work_layout(int n_in, int n_hidden, int n_layers, int n_out, int batch_norm, long n) {
    Work w{};
    long at = 0;
    for (int l = 0; l <= n_layers; ++l) {
        w.a[l] = at;
        at += round4((long)(l == 0 ? n_in : n_hidden) * n);
    }
    w.p = at;
    at += round4((long)n_out * n);
    const long widest = n_hidden > n_out ? n_hidden : n_out;
    for (int i = 0; i < 2; ++i) {
        w.dz[i] = at;
        at += round4(widest * n);
    }
    if (batch_norm) {
        for (int l = 0; l < n_layers; ++l) {
            w.xhat[l] = at;
            at += round4((long)n_hidden * n);
            w.invstd[l] = at;
            at += round4(n_hidden);
        }
    }
    w.total = at;
    return w;
}

int check_params(const bmpc_policy_train_t *net, const bmpc_policy_params_t &q, const char *name) {
    for (int l = 0; l <= net->n_layers; ++l) {
        if (!q.W[l]) return bad(std::string("null array: ") + name + ".W[" + std::to_string(l) + "]");
        if (!q.b[l]) return bad(std::string("null array: ") + name + ".b[" + std::to_string(l) + "]");
        if (net->batch_norm && l < net->n_layers) {
            if (!q.gamma[l]) return bad(std::string("null array: ") + name + ".gamma[" + std::to_string(l) + "]");
            if (!q.beta[l]) return bad(std::string("null array: ") + name + ".beta[" + std::to_string(l) + "]");
        }
    }
    return BMPC_OK;
}

int check_net(const bmpc_policy_train_t *net, bool moments) {
    if (!net) return bad("null network descriptor (bmpc_policy_train_t)");
    if (net->n_in < 1 || net->n_in > BMPC_POLICY_MAX_WIDTH) return bad("n_in must be in [1, 512], got " + std::to_string(net->n_in));
    if (net->n_hidden < 1 || net->n_hidden > BMPC_POLICY_MAX_WIDTH) return bad("n_hidden must be in [1, 512], got " + std::to_string(net->n_hidden));
    if (net->n_layers < 1 || net->n_layers > BMPC_POLICY_MAX_LAYERS) return bad("n_layers must be in [1, 8], got " + std::to_string(net->n_layers));
    if (net->n_out < 1 || net->n_out > BMPC_POLICY_MAX_OUT) return bad("n_out must be in [1, 64], got " + std::to_string(net->n_out));
    if (int rc = check_params(net, net->p, "p")) return rc;
    if (moments) {
        if (int rc = check_params(net, net->m, "m")) return rc;
        if (int rc = check_params(net, net->v, "v")) return rc;
    }
    if (net->batch_norm) {
        if (!(net->eps >= 0.0) || !std::isfinite(net->eps)) return bad("eps must be finite and not negative, got " + std::to_string(net->eps));
        for (int l = 0; l < net->n_layers; ++l) {
            if (!net->running_mean[l]) return bad("null array: running_mean[" + std::to_string(l) + "]");
            if (!net->running_var[l]) return bad("null array: running_var[" + std::to_string(l) + "]");
        }
    }
    return BMPC_OK;
}

int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(BMPC_DEVICE_ERROR, std::string("policy training step, ") + what + " kernel: " + hipGetErrorString(e));
    return BMPC_OK;
}

float *f32(void *p) { return static_cast<float *>(p); }

}  // namespace
}  // namespace bunmpc

extern "C" int bmpc_policy_params_struct_size(void) { return (int)sizeof(bmpc_policy_params_t); }
extern "C" int bmpc_policy_train_struct_size(void) { return (int)sizeof(bmpc_policy_train_t); }
extern "C" int bmpc_policy_step_struct_size(void) { return (int)sizeof(bmpc_policy_step_t); }
extern "C" int bmpc_policy_train_tile(void) { return bunmpc::kThreads; }

extern "C" long bmpc_policy_train_work_bytes(int n_in, int n_hidden, int n_layers, int n_out, int batch_norm, long n) {
    if (!bunmpc::sizes_ok(n_in, n_hidden, n_layers, n_out) || n < 1 || n > BMPC_POLICY_TRAIN_MAX_ROWS) return -1;
    return 4 * bunmpc::work_layout(n_in, n_hidden, n_layers, n_out, batch_norm, n).total;
}

extern "C" int bmpc_policy_train_step_device(const bmpc_policy_train_t *net, const bmpc_policy_step_t *step, void *hip_stream) {
    using namespace bunmpc;
    if (int rc = check_net(net, true)) return rc;
    if (!step) return bad("null step descriptor (bmpc_policy_step_t)");
    if (step->n < 1 || step->n > BMPC_POLICY_TRAIN_MAX_ROWS) return bad("n must be in [1, 1024], got " + std::to_string(step->n));
    if (net->batch_norm && step->n < 2) return bad("n must be 2 at least with batch_norm (the batch's variance), got 1");
    if (!step->x) return bad("null input array: x");
    if (!step->y) return bad("null input array: y");
    if (step->x_stride < net->n_in) return bad("x_stride must be n_in = " + std::to_string(net->n_in) + " at least, got " + std::to_string(step->x_stride));
    if (step->y_stride < net->n_out) return bad("y_stride must be n_out = " + std::to_string(net->n_out) + " at least, got " + std::to_string(step->y_stride));
    if (!step->loss) return bad("null output: loss");
    if (!std::isfinite(step->lr)) return bad("lr must be finite, got " + std::to_string(step->lr));
    if (!(step->bc1 > 0.0) || !std::isfinite(step->bc1)) return bad("bc1 must be positive and finite, got " + std::to_string(step->bc1));
    if (!(step->bc2 > 0.0) || !std::isfinite(step->bc2)) return bad("bc2 must be positive and finite, got " + std::to_string(step->bc2));
    if (step->grads)
        if (int rc = check_params(net, *step->grads, "grads")) return rc;
    const int n = (int)step->n, L = net->n_layers, H = net->n_hidden, bn = net->batch_norm ? 1 : 0;
    const Work w = work_layout(net->n_in, H, L, net->n_out, bn, n);
    if (!net->work) return bad("null scratch: work");
    if (reinterpret_cast<uintptr_t>(net->work) & 15) return bad("work must be 16-byte aligned");
    if (net->work_bytes < 4 * w.total)
        return bad("work_bytes must be bmpc_policy_train_work_bytes(...) = " + std::to_string(4 * w.total) + " at least for n = " + std::to_string(n) + ", got " + std::to_string(net->work_bytes));

    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    float *work = f32(net->work);
    Adam adam;
    adam.w1 = (float)(1.0 - 0.9);
    adam.w2 = (float)(1.0 - 0.999);
    adam.b2 = (float)0.999;
    adam.step = (float)(step->lr / step->bc1);
    adam.root = (float)std::sqrt(step->bc2);
    adam.eps = (float)1e-8;
    const bmpc_policy_params_t *g = step->grads;

    const long cells = (long)n * net->n_in;
    hipLaunchKernelGGL(train_input_kernel, dim3((unsigned)((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, step->x, step->x_stride, n, net->n_in, work + w.a[0]);
    if (int rc = launched("input")) return rc;
    for (int l = 0; l <= L; ++l) {
        Forward f{};
        f.W = f32(net->p.W[l]);
        f.b = f32(net->p.b[l]);
        f.aT = work + w.a[l];
        f.K = l == 0 ? net->n_in : H;
        f.N = l == L ? net->n_out : H;
        f.n = n;
        f.last = l == L;
        f.bn = bn && l < L;
        f.outT = work + (l == L ? w.p : w.a[l + 1]);
        if (f.bn) {
            f.xhatT = work + w.xhat[l];
            f.invstd = work + w.invstd[l];
            f.gamma = f32(net->p.gamma[l]);
            f.beta = f32(net->p.beta[l]);
            f.running_mean = f32(net->running_mean[l]);
            f.running_var = f32(net->running_var[l]);
            f.eps = (float)net->eps;
        }
        hipLaunchKernelGGL(train_forward_kernel, dim3((unsigned)((f.N + kCols - 1) / kCols)), dim3(kThreads), 0, stream, f);
        if (int rc = launched("forward")) return rc;
    }
    int cur = 0;
    hipLaunchKernelGGL(train_loss_kernel, dim3(1), dim3(kThreads), 0, stream, work + w.p, step->y, step->y_stride, n, net->n_out, work + w.dz[cur], step->loss);
    if (int rc = launched("loss")) return rc;
    for (int l = L; l >= 0; --l) {
        const int K = l == 0 ? net->n_in : H, N = l == L ? net->n_out : H;
        if (l > 0) {
            Below f{};
            f.W = f32(net->p.W[l]);
            f.dzT = work + w.dz[cur];
            f.aT = work + w.a[l];
            f.outT = work + w.dz[cur ^ 1];
            f.K = K;
            f.N = N;
            f.n = n;
            f.bn = bn;
            f.adam = adam;
            if (bn) {
                f.xhatT = work + w.xhat[l - 1];
                f.invstd = work + w.invstd[l - 1];
                f.gamma = f32(net->p.gamma[l - 1]);
                f.beta = f32(net->p.beta[l - 1]);
                f.m_gamma = f32(net->m.gamma[l - 1]);
                f.m_beta = f32(net->m.beta[l - 1]);
                f.v_gamma = f32(net->v.gamma[l - 1]);
                f.v_beta = f32(net->v.beta[l - 1]);
                f.g_gamma = g ? f32(g->gamma[l - 1]) : nullptr;
                f.g_beta = g ? f32(g->beta[l - 1]) : nullptr;
            }
            hipLaunchKernelGGL(train_below_kernel, dim3((unsigned)((K + kCols - 1) / kCols)), dim3(kThreads), 0, stream, f);
            if (int rc = launched("da")) return rc;
        }
        Weights f{};
        f.dzT = work + w.dz[cur];
        f.aT = work + w.a[l];
        f.W = f32(net->p.W[l]);
        f.b = f32(net->p.b[l]);
        f.m_W = f32(net->m.W[l]);
        f.m_b = f32(net->m.b[l]);
        f.v_W = f32(net->v.W[l]);
        f.v_b = f32(net->v.b[l]);
        f.g_W = g ? f32(g->W[l]) : nullptr;
        f.g_b = g ? f32(g->b[l]) : nullptr;
        f.K = K;
        f.N = N;
        f.n = n;
        f.adam = adam;
        hipLaunchKernelGGL(train_weights_kernel, dim3((unsigned)((K + 15) / 16), (unsigned)((N + 15) / 16)), dim3(kThreads), 0, stream, f);
        if (int rc = launched("dW")) return rc;
        cur ^= 1;
    }
    return BMPC_OK;
}

extern "C" int bmpc_policy_pack_device(const bmpc_policy_train_t *net, void *packed, long packed_bytes, void *hip_stream) {
    using namespace bunmpc;
    if (int rc = check_net(net, false)) return rc;
    Pack f{};
    long at = 0, most = 0;
    for (int l = 0; l <= net->n_layers; ++l) {
        const bool bn = net->batch_norm && l < net->n_layers;
        const long floats = layer_floats(l == 0 ? net->n_in : net->n_hidden, l == net->n_layers ? net->n_out : net->n_hidden, bn);
        f.at[l] = at;
        at += floats;
        most = floats > most ? floats : most;
        f.W[l] = f32(net->p.W[l]);
        f.b[l] = f32(net->p.b[l]);
        if (bn) {
            f.gamma[l] = f32(net->p.gamma[l]);
            f.beta[l] = f32(net->p.beta[l]);
            f.running_mean[l] = f32(net->running_mean[l]);
            f.running_var[l] = f32(net->running_var[l]);
        }
    }
    if (packed_bytes != 4 * at) return bad("packed_bytes must be bmpc_policy_packed_bytes(...) = " + std::to_string(4 * at) + ", got " + std::to_string(packed_bytes));
    if (!packed) return bad("null packed image: packed");
    if (reinterpret_cast<uintptr_t>(packed) & 15) return bad("packed must be 16-byte aligned");
    f.n_in = net->n_in;
    f.n_hidden = net->n_hidden;
    f.n_layers = net->n_layers;
    f.n_out = net->n_out;
    f.batch_norm = net->batch_norm;
    f.eps = net->eps;
    f.image = f32(packed);
    hipLaunchKernelGGL(policy_pack_kernel, dim3((unsigned)((most + kThreads - 1) / kThreads), (unsigned)(net->n_layers + 1)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(hip_stream), f);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(BMPC_DEVICE_ERROR, std::string("policy pack kernel: ") + hipGetErrorString(e));
    return BMPC_OK;
}
