// TEST ONLY: the lane helpers of the centroidal kernels (biconvex_lanes.h) called on a test's own inputs, group by group, so that each can
// be held to its model bit for bit (bmpc_probe_lanes, include/bunmpc.h: the layouts; tests/lanes_np.py: the models;
// tests/test_lane_probe_gpu.py).  No helper is restated here: the kernel calls them, at every LPP a kernel instantiates them with, and
// this unit is built with the fp64 units' flags (bunmpc_amd/build.py), so the helpers are compiled as they are there.  A wave is a
// workgroup of 64 threads and one test case: word [k][lane] of its NIN input rows, word [k][lane] of its NOUT output rows.
#include "../../include/bunmpc.h"
#include "biconvex_kernels.h"

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"

typedef unsigned long long word_t;
__device__ __forceinline__ word_t bits(double v) { return (word_t)__double_as_longlong(v); }
__device__ __forceinline__ word_t bits(float v) { return (word_t)__float_as_uint(v); }
__device__ __forceinline__ word_t bits(bool v) { return v ? 1ull : 0ull; }
__device__ __forceinline__ double as_double(word_t w) { return __longlong_as_double((long long)w); }
__device__ __forceinline__ float as_float(word_t w) { return __uint_as_float((unsigned)w); }
// lane 0's word, in scalar registers
__device__ __forceinline__ word_t uniform_word(const word_t *row) {
    const word_t w = row[0];
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(w >> 32)), lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)w);
    return ((word_t)hi << 32) | lo;
}

// o: the lane's word of the group's first output row for this L; rows are 64 words apart
template <int L> __device__ __forceinline__ void probe_sum64(double a, double b, word_t *o) {
    o[0] = bits(seg_sum<L>(a));
    double x = a, y = b;
    seg_sum2<L>(x, y);
    o[64] = bits(x);
    o[128] = bits(y);
    double z = a;
    seg_sum1<L>(z);
    o[192] = bits(z);
}
template <int L> __device__ __forceinline__ void probe_sum32(float a, float b, word_t *o) {
    float x = a, y = b;
    seg_sum2_f32<L>(x, y);
    o[0] = bits(x);
    o[64] = bits(y);
    float z = a;
    seg_sum1_f32<L>(z);
    o[128] = bits(z);
}

// rows of 64 words a wave of the group reads (out = false) or writes; 0: no such group
__host__ __device__ constexpr int probe_rows(int group, bool out) {
    switch (group) {
    case BMPC_PROBE_SUM64: return out ? 16 : 2;
    case BMPC_PROBE_SUM32: return out ? 9 : 2;
    case BMPC_PROBE_SHIFT: return out ? 4 : 2;
    case BMPC_PROBE_MASK: return out ? 9 : 2;
    case BMPC_PROBE_THETA: return out ? 1 : 2;
    case BMPC_PROBE_ARITH: return out ? 17 : 7;
    case BMPC_PROBE_BANDED: return out ? 3 : 4;
    default: return 0;
    }
}

__global__ __launch_bounds__(64) void lane_probe_kernel(int group, const word_t *in_all, word_t *out_all) {
    __shared__ double rec[64 * 6];
    const int lane = threadIdx.x;
    const word_t *in = in_all + (size_t)blockIdx.x * 64 * probe_rows(group, false);       // (wave-uniform)
    word_t *out = out_all + (size_t)blockIdx.x * 64 * probe_rows(group, true) + lane;
    switch (group) {
    case BMPC_PROBE_SUM64: {
        const double a = as_double(in[lane]), b = as_double(in[64 + lane]);
        probe_sum64<16>(a, b, out);
        probe_sum64<21>(a, b, out + 4 * 64);
        probe_sum64<32>(a, b, out + 8 * 64);
        probe_sum64<64>(a, b, out + 12 * 64);
    } break;
    case BMPC_PROBE_SUM32: {
        const float a = as_float(in[lane]), b = as_float(in[64 + lane]);
        probe_sum32<16>(a, b, out);
        probe_sum32<32>(a, b, out + 3 * 64);
        probe_sum32<64>(a, b, out + 6 * 64);
    } break;
    case BMPC_PROBE_SHIFT: {
        const double d = as_double(in[lane]);
        const float f = as_float(in[64 + lane]);
        out[0] = bits(from_prev(d));
        out[64] = bits(from_next(d));
        out[128] = bits(from_prev(f));
        out[192] = bits(from_next(f));
    } break;
    case BMPC_PROBE_MASK: {
        const mask_t m = uniform_word(in), need = uniform_word(in + 64);
        out[0] = seg_uniform<21>(m & seg_desig<21>());
        out[64] = bits(seg_covered<16>(m, need));
        out[128] = bits(seg_covered<32>(m, need));
        out[192] = bits(seg_covered<64>(m, need));
        unsigned d0, d1;
        seg_dead32(need, d0, d1);
        out[256] = d0;
        out[320] = d1;
        out[384] = bits(seg_covered32(m, d0, d1));
        const bool mine = lanes(m);
        out[448] = bits(mine);
        out[512] = __ballot(mine);
    } break;
    case BMPC_PROBE_THETA: {
        const double *tol2 = reinterpret_cast<const double *>(in), *floor2 = tol2 + 64;
        double mine = 0.0;
        for (int j = 0; j < 64; ++j) {      // (screen_theta is wave-uniform: one case per turn, kept by lane j)
            const double th = screen_theta(tol2[j], floor2[j]);
            mine = lane == j ? th : mine;
        }
        out[0] = bits(mine);
    } break;
    case BMPC_PROBE_ARITH: {
        const double *in_a = reinterpret_cast<const double *>(in), *in_b = in_a + 64;
        const double a = in_a[lane], b = in_b[lane], c = as_double(in[128 + lane]);
        const word_t flags = in[192 + lane];
        const int m = (int)(unsigned)flags;
        const bool ok = (flags >> 32) & 1;
        const float fa = as_float(in[256 + lane]), fb = as_float(in[320 + lane]), fc = as_float(in[384 + lane]);
        out[0] = bits(keep_if(a, m));
        out[64] = bits(keep_if(fa, m));
        out[128] = bits(fma3(a, b, c));
        out[192] = bits(fma3_s(uniform_load(in_a, 0u), b, c));
        out[256] = bits(clamp_box(a, b, c));
        out[320] = bits(clamp_box(fa, fb, fc));
        double *mine = rec + 6 * lane;
        mine[0] = a; mine[1] = b; mine[2] = c; mine[3] = a; mine[4] = b; mine[5] = c;
        __syncthreads();
        double v[6];
        lds_block<6>(mine, v, ok);
        for (int l = 0; l < 6; ++l) out[(6 + l) * 64] = bits(v[l]);
        out[12 * 64] = bits(ldz<double>(in_a, 8u * (unsigned)lane, 0, ok));
        out[13 * 64] = bits(ldz<float>(in_a, 8u * (unsigned)lane, 0, ok));
        double u = 0.0;
        for (unsigned j = 0; j < 64; ++j) {      // (uniform_load takes a wave-uniform index: one element per turn, kept by lane j)
            const double t = uniform_load(in_b, j);
            u = (unsigned)lane == j ? t : u;
        }
        out[14 * 64] = bits(u);
        out[15 * 64] = bits(fast_div(a, b));
        out[16 * 64] = bits(fast_div(fa, fb));
    } break;
    case BMPC_PROBE_BANDED: {
        const double g2 = as_double(in[lane]), cv = as_double(in[64 + lane]);
        const double Lh = as_double(uniform_word(in + 128)), tol2 = as_double(uniform_word(in + 192));
        bool retry = false, finished = false;
        const bool clear = banded_decisions(g2, cv, Lh, tol2, retry, finished);
        out[0] = bits(clear);
        out[64] = bits(retry);
        out[128] = bits(finished);
    } break;
    default: break;
    }
}

// The quad stage of the certified loops' screen (quad_sum_f32, quad_theta_f32, quad_screen), in a kernel of its own: lane_probe_kernel and
// its seven groups stay the instructions they were.  NIN 2: the lane's partial g2 and a theta per lane, doubles; NOUT 3: quad_sum_f32(g2)
// and quad_theta_f32(theta) as floats, and the ballot of quad_screen(g2, theta) (every lane writes the wave's word).
constexpr int kQuadProbeIn = 2, kQuadProbeOut = 3;
__global__ __launch_bounds__(64) void quad_probe_kernel(const word_t *in_all, word_t *out_all) {
    const int lane = threadIdx.x;
    const word_t *in = in_all + (size_t)blockIdx.x * 64 * kQuadProbeIn;
    word_t *out = out_all + (size_t)blockIdx.x * 64 * kQuadProbeOut + lane;
    const double g2 = as_double(in[lane]), theta = as_double(in[64 + lane]);
    out[0] = bits(quad_sum_f32(g2));
    out[64] = bits(quad_theta_f32(theta));
    out[128] = quad_screen(g2, theta);
}

}  // namespace

bool lane_probe_words(int group, int *nin, int *nout) {
    *nin = probe_rows(group, false);
    *nout = probe_rows(group, true);
    return *nin != 0;
}

hipError_t launch_lane_probe(int group, const unsigned long long *in, unsigned long long *out, long waves, hipStream_t stream) {
    hipLaunchKernelGGL(lane_probe_kernel, dim3((unsigned)waves), dim3(64), 0, stream, group, in, out);
    return hipGetLastError();
}

}  // namespace bunmpc

// TEST ONLY, and in no header of include/: the tables of those headers are held to their recorded sizes, and bmpc_probe_lanes to its seven
// groups, by tests/test_abi_cpu.py and tests/test_lane_probe_cpu.py, so the probe of the quad stage has an entry point of its own that
// tests/test_quad_screen_gpu.py binds by name.  in / out are HOST arrays of 64-bit words laid out as bmpc_probe_lanes lays them out:
// in [waves][2][64], out [waves][3][64] (quad_probe_kernel above).  BMPC_BAD_ARG before any device call, as there.
extern "C" int bmpc_probe_quad_screen(const void *in, long in_bytes, void *out, long out_bytes) {
    using namespace bunmpc;
    const long wave_in = 512L * kQuadProbeIn, wave_out = 512L * kQuadProbeOut;
    if (!in || !out || in_bytes < wave_in || in_bytes % wave_in != 0 || in_bytes / wave_in > (1L << 20)) return BMPC_BAD_ARG;
    const long waves = in_bytes / wave_in;
    if (out_bytes != waves * wave_out) return BMPC_BAD_ARG;
    unsigned long long *din = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&din), (size_t)(in_bytes + out_bytes)) != hipSuccess) return BMPC_DEVICE_ERROR;
    unsigned long long *dout = din + in_bytes / 8;
    bool ok = hipMemcpy(din, in, (size_t)in_bytes, hipMemcpyHostToDevice) == hipSuccess && hipMemset(dout, 0, (size_t)out_bytes) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(quad_probe_kernel, dim3((unsigned)waves), dim3(64), 0, nullptr, din, dout);
        ok = hipGetLastError() == hipSuccess && hipMemcpy(out, dout, (size_t)out_bytes, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(din);
    return ok ? BMPC_OK : BMPC_DEVICE_ERROR;
}
