// TEST ONLY: the SE(3) primitives of rbd_device.h called on a test's own rows, one thread per row, so that each can be held to a reference
// that shares no formula with it (tests/golden/lie_ref.npz, written at 60 digits by tests/golden/make_golden_lie.py;
// tests/test_lie_ref_gpu.py).  No routine is restated here, and this unit is built with ik_ddp.hip's flags (bunmpc_amd/build.py), so the
// inlined routines are contracted as they are in the solver.  The state operators see a state whose joints and velocities are zero: their
// base blocks are what is probed (the other rows are plain additions, tests/test_rbd_gpu.py).
#include "../../include/bunmpc.h"
#include "ik_types.h"
#include "rbd_device.h"

namespace bunmpc {
namespace {

enum LieOp { kSincos, kRcpRsqrt, kAtan2Pos, kExp6, kJexp3, kJlog3, kQLeft, kJexp6, kLog3Q, kDiff, kIntegrate, kLieOps };

// doubles a row of the op reads (out = false) or writes; 0: no such op
__host__ __device__ constexpr int lie_width(int op, bool out) {
    switch (op) {
    case kSincos: return out ? 2 : 1;
    case kRcpRsqrt: return out ? 2 : 1;
    case kAtan2Pos: return out ? 1 : 2;
    case kExp6: return out ? 12 : 6;
    case kJexp3: return out ? 9 : 3;
    case kJlog3: return out ? 9 : 3;
    case kQLeft: return out ? 9 : 6;
    case kJexp6: return out ? 36 : 6;
    case kLog3Q: return out ? 3 : 4;
    case kDiff: return out ? 48 : 14;           // p0, q0, p1, q1 -> state_diff_q (6), state_diff<false> (6), the Jl of state_diff<true> (36)
    case kIntegrate: return out ? 14 : 13;      // p, q, dx (6) -> state_integrate_q (7), state_integrate (7)
    default: return 0;
    }
}

__global__ __launch_bounds__(64) void lie_probe_kernel(int op, const double *in_all, double *out_all, int n) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= n) return;
    const double *in = in_all + (size_t)row * lie_width(op, false);
    double *out = out_all + (size_t)row * lie_width(op, true);
    switch (op) {
    case kSincos: rbd::sincos_fast(in[0], out[0], out[1]); break;
    case kRcpRsqrt: out[0] = rbd::rcp_fast(in[0]); out[1] = rbd::rsqrt_fast(in[0]); break;
    case kAtan2Pos: out[0] = rbd::atan2_pos(in[0], in[1]); break;
    case kExp6: rbd::exp6(in, out, out + 9); break;
    case kJexp3: rbd::jexp3(in, out); break;
    case kJlog3: rbd::jlog3(in, out); break;
    case kQLeft: rbd::q_left(in, in + 3, out); break;
    case kJexp6: rbd::jexp6(in, out); break;
    case kLog3Q: {
        double R[9];
        rbd::quat_to_R(in, R);
        rbd::log3(R, out);
    } break;
    case kDiff: {
        double x0[kNX], x1[kNX], d[kNDX];
        for (int i = 0; i < kNX; ++i) { x0[i] = i < 7 ? in[i] : 0.0; x1[i] = i < 7 ? in[7 + i] : 0.0; }
        rbd::state_diff_q(x0, x1, d);
        for (int i = 0; i < 6; ++i) out[i] = d[i];
        rbd::state_diff<false>(x0, x1, d, nullptr);
        for (int i = 0; i < 6; ++i) out[6 + i] = d[i];
        rbd::state_diff<true>(x0, x1, d, out + 12);
    } break;
    case kIntegrate: {
        double x[kNX], dx[kNDX], xn[kNX];
        for (int i = 0; i < kNX; ++i) x[i] = i < 7 ? in[i] : 0.0;
        for (int i = 0; i < kNDX; ++i) dx[i] = i < 6 ? in[7 + i] : 0.0;
        rbd::state_integrate_q(x, dx, xn);
        for (int i = 0; i < 7; ++i) out[i] = xn[i];
        rbd::state_integrate(x, dx, xn);
        for (int i = 0; i < 7; ++i) out[7 + i] = xn[i];
    } break;
    default: break;
    }
}

}  // namespace
}  // namespace bunmpc

// TEST ONLY, and in no header of include/ (their tables are held to their recorded sizes by tests/test_abi_cpu.py):
// tests/test_lie_ref_gpu.py binds it by name.  in / out are HOST arrays of n rows of the op's widths (lie_width above; the ops in the order
// of LieOp); one launch of ceil(n / 64) blocks of 64 threads.  BMPC_BAD_ARG, before any device call, for an op that does not exist, a null
// pointer, n < 1 or more than 2^20 rows, or sizes that are not n times the op's widths.
extern "C" int bmpc_probe_lie(int op, const double *in, long in_doubles, double *out, long out_doubles, int n) {
    using namespace bunmpc;
    if (op < 0 || op >= kLieOps || !in || !out || n < 1 || n > (1 << 20)) return BMPC_BAD_ARG;
    const long win = lie_width(op, false), wout = lie_width(op, true);
    if (in_doubles != n * win || out_doubles != n * wout) return BMPC_BAD_ARG;
    double *din = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&din), (size_t)(in_doubles + out_doubles) * sizeof(double)) != hipSuccess) return BMPC_DEVICE_ERROR;
    double *dout = din + in_doubles;
    bool ok = hipMemcpy(din, in, (size_t)in_doubles * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemset(dout, 0xff, (size_t)out_doubles * sizeof(double)) == hipSuccess;      // (all ones: a NaN where a row writes nothing)
    if (ok) {
        hipLaunchKernelGGL(lie_probe_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, op, din, dout, n);
        ok = hipGetLastError() == hipSuccess && hipMemcpy(out, dout, (size_t)out_doubles * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(din);
    return ok ? BMPC_OK : BMPC_DEVICE_ERROR;
}
