// The kernels of the batched centroidal ADMM and their launches, templated on the number of feet E.  Included inside the anonymous
// namespace of one translation unit per foot count and precision (after biconvex_lanes.h and biconvex_admm_body.h):
//   biconvex_admm.hip        fp64, E = 4        biconvex_admm_f32.hip      fp32, E = 4
//   biconvex_admm_e2.hip     fp64, E = 2        biconvex_admm_f32_e2.hip   fp32, E = 2
// so that every unit is built with its own flags (bunmpc_amd/build.py) and the units build in parallel.  Which kernel a batch gets is
// decided once, for every E, by launch_biconvex_admm (biconvex_admm.hip).
#pragma once

// fp64, WPE = 1: ONE wave per SIMD.  The body holds 294 registers; capped at 256 with the FISTA iterates in registers the compiler parks
// 63 of them in scratch memory, some inside the loops (round 2 measured that build 4 % faster at 14 x the HBM traffic, round 3 level).
// WPE = 2 (round 4): two waves per SIMD with x_k and its image in LDS (biconvex_admm_body.h: XLDS) -- both FISTA loops free of
// scratch accesses at 256 registers, the two waves of a SIMD covering each other's latencies.  A lone wave of this build is slower
// than a lone wave of the other (2.30 against 1.94 ms: the LDS round trip sits on its chain), so it is taken where the batch
// needs more waves than the chip has SIMDs and three problems per wave do not save a round (launch_biconvex_admm):
// B = 4096, H = 20: 3.74 against 4.02 ms.
template <typename R, int LPP, int E, bool RAW, bool HASQF, int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void biconvex_admm_kernel(const BatchArgs a) {
    admm_body<R, LPP, E, RAW, HASQF, false, WPE == 2>(a);
}
// horizons of 64 .. 255 knots: one problem per workgroup of WAVES waves (biconvex_admm_body.h: WAVES)
template <int E, int WAVES, bool RAW, bool HASQF, int WPE>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void biconvex_admm_wg_kernel(const BatchArgs a) {
    admm_body<double, 64, E, RAW, HASQF, false, WPE == 2, WAVES>(a);
}
// the work-stealing variant (biconvex_admm_body.h: STEAL): three problems per wave, harness form, fp64
template <int E, int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void biconvex_admm_steal_kernel(const BatchArgs a) {
    admm_body<double, 21, E, false, false, true, WPE == 2>(a);
}
// fp32: TWO waves per SIMD -- this latency-bound loop gains a second wave to issue from while the first waits (one wave per SIMD:
// 9.0 ms).  Instantiated only in the fp32 units (biconvex_admm_f32.hip explains their flags).
template <int LPP, int E>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void biconvex_admm_kernel_f32(const BatchArgs a) {
    admm_body<float, LPP, E, false, false>(a);
}

// LDS of one problem: the x_init rows' multipliers and the header, then one record per knot (X, P, F, R)
template <int E>
size_t problem_lds(int H) { return (size_t)kSegLds + (size_t)knot_lds(E) * (size_t)(H + 1); }

template <typename R, int LPP, int E, bool RAW, bool HASQF>
hipError_t launch(const BatchArgs &a, bool two_per_simd, hipStream_t stream) {
    const int per_wave = 64 / LPP;
    const unsigned grid = (unsigned)((a.B + per_wave - 1) / per_wave);
    const size_t lds = sizeof(R) * (kLdsZeros + per_wave * problem_lds<E>(a.H));
    if (sizeof(R) == sizeof(float))      // biconvex_admm_f32.hip, biconvex_admm_f32_e2.hip
        return E == 4 ? launch_biconvex_admm_f32(a, LPP, grid, lds, stream) : launch_biconvex_admm_f32_e2(a, LPP, grid, lds, stream);
    if (two_per_simd) hipLaunchKernelGGL((biconvex_admm_kernel<double, LPP, E, RAW, HASQF, 2>), dim3(grid), dim3(64), lds, stream, a);
    else hipLaunchKernelGGL((biconvex_admm_kernel<double, LPP, E, RAW, HASQF, 1>), dim3(grid), dim3(64), lds, stream, a);
    return hipGetLastError();
}

template <int E, int WAVES, bool RAW, bool HASQF, int WPE>
hipError_t launch_wg(const BatchArgs &a, hipStream_t stream) {
    const size_t lds = sizeof(double) * (kLdsZeros + problem_lds<E>(a.H) + (size_t)WAVES * 40);
    static std::once_flag once;      // (more than the 64 KB a kernel may take without asking, from 209 knots on)
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] { attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&biconvex_admm_wg_kernel<E, WAVES, RAW, HASQF, WPE>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024); });
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL((biconvex_admm_wg_kernel<E, WAVES, RAW, HASQF, WPE>), dim3((unsigned)a.B), dim3(64 * WAVES), lds, stream, a);
    return hipGetLastError();
}
template <int E, int WAVES, int WPE>
hipError_t launch_wg_form(const BatchArgs &a, hipStream_t stream) {
    if (a.precision != 0) return hipErrorInvalidValue;      // (fp64 only)
    if (!a.raw) return launch_wg<E, WAVES, false, false, WPE>(a, stream);
    return a.qf ? launch_wg<E, WAVES, true, true, WPE>(a, stream) : launch_wg<E, WAVES, true, false, WPE>(a, stream);
}

// the persistent grid of the work-stealing kernel (a.queue: its device counter, set by the caller)
template <int E>
hipError_t launch_steal(const BatchArgs &a, long waves, bool two_per_simd, hipStream_t stream) {
    const size_t lds = sizeof(double) * (kLdsZeros + 3 * problem_lds<E>(a.H));
    if (two_per_simd) hipLaunchKernelGGL((biconvex_admm_steal_kernel<E, 2>), dim3((unsigned)waves), dim3(64), lds, stream, a);
    else hipLaunchKernelGGL((biconvex_admm_steal_kernel<E, 1>), dim3((unsigned)waves), dim3(64), lds, stream, a);
    return hipGetLastError();
}

template <int LPP, int E>
hipError_t launch_lpp(const BatchArgs &a, bool two_per_simd, hipStream_t stream) {
    if (a.precision == 1) {   // fp32 arithmetic: harness form only
        if (a.raw || LPP == 21) return hipErrorInvalidValue;
        return launch<float, LPP == 21 ? 32 : LPP, E, false, false>(a, false, stream);
    }
    if (!a.raw) return launch<double, LPP, E, false, false>(a, two_per_simd, stream);
    return a.qf ? launch<double, LPP, E, true, true>(a, two_per_simd, stream) : launch<double, LPP, E, true, false>(a, two_per_simd, stream);
}

// the launch launch_biconvex_admm decided on
template <int E>
hipError_t launch_admm(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream) {
    if (l.steal) return launch_steal<E>(a, l.steal_waves, l.w2, stream);
    switch (l.lpp) {
        case 16: return launch_lpp<16, E>(a, l.w2, stream);
        case 21: return launch_lpp<21, E>(a, l.w2, stream);
        case 32: return launch_lpp<32, E>(a, l.w2, stream);
        case 64: return launch_lpp<64, E>(a, l.w2, stream);
        case 128: return l.w2 ? launch_wg_form<E, 2, 2>(a, stream) : launch_wg_form<E, 2, 1>(a, stream);
        case 192: return l.w2 ? launch_wg_form<E, 3, 2>(a, stream) : launch_wg_form<E, 3, 1>(a, stream);
        case 256: return l.w2 ? launch_wg_form<E, 4, 2>(a, stream) : launch_wg_form<E, 4, 1>(a, stream);
        default: return hipErrorInvalidValue;
    }
}

// private-segment (scratch) bytes per lane, the largest over the kernels listed
template <typename... K>
int max_scratch_bytes(K... kernels) {
    size_t worst = 0;
    for (const void *k : {reinterpret_cast<const void *>(kernels)...}) {
        hipFuncAttributes at;
        if (hipFuncGetAttributes(&at, k) != hipSuccess) return -1;
        worst = at.localSizeBytes > worst ? at.localSizeBytes : worst;
    }
    return (int)worst;
}
// ... of the fp64 instantiations of one foot count: batch kernel (every lanes-per-problem, form and build), workgroup, work stealing
template <int E, int LPP>
int lpp_scratch_bytes() {
    return max_scratch_bytes(&biconvex_admm_kernel<double, LPP, E, false, false, 1>, &biconvex_admm_kernel<double, LPP, E, true, false, 1>,
                             &biconvex_admm_kernel<double, LPP, E, true, true, 1>, &biconvex_admm_kernel<double, LPP, E, false, false, 2>,
                             &biconvex_admm_kernel<double, LPP, E, true, false, 2>, &biconvex_admm_kernel<double, LPP, E, true, true, 2>);
}
template <int E, int WAVES>
int wg_scratch_bytes() {
    return max_scratch_bytes(&biconvex_admm_wg_kernel<E, WAVES, false, false, 1>, &biconvex_admm_wg_kernel<E, WAVES, true, false, 1>,
                             &biconvex_admm_wg_kernel<E, WAVES, true, true, 1>, &biconvex_admm_wg_kernel<E, WAVES, false, false, 2>,
                             &biconvex_admm_wg_kernel<E, WAVES, true, false, 2>, &biconvex_admm_wg_kernel<E, WAVES, true, true, 2>);
}
template <int E>
int admm_scratch_bytes() {
    int worst = max_scratch_bytes(&biconvex_admm_steal_kernel<E, 1>, &biconvex_admm_steal_kernel<E, 2>);
    for (int s : {lpp_scratch_bytes<E, 16>(), lpp_scratch_bytes<E, 21>(), lpp_scratch_bytes<E, 32>(), lpp_scratch_bytes<E, 64>(),
                  wg_scratch_bytes<E, 2>(), wg_scratch_bytes<E, 3>(), wg_scratch_bytes<E, 4>()}) {
        if (s < 0 || worst < 0) return -1;
        worst = s > worst ? s : worst;
    }
    return worst;
}

// fp32 (the units built without the SLP vectoriser)
template <int E>
hipError_t launch_f32(const BatchArgs &a, int lpp, unsigned grid, size_t lds, hipStream_t stream) {
    if (lpp == 16) hipLaunchKernelGGL((biconvex_admm_kernel_f32<16, E>), dim3(grid), dim3(64), lds, stream, a);
    else if (lpp == 32) hipLaunchKernelGGL((biconvex_admm_kernel_f32<32, E>), dim3(grid), dim3(64), lds, stream, a);
    else if (lpp == 64) hipLaunchKernelGGL((biconvex_admm_kernel_f32<64, E>), dim3(grid), dim3(64), lds, stream, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
template <int E>
int f32_scratch_bytes() { return max_scratch_bytes(&biconvex_admm_kernel_f32<16, E>, &biconvex_admm_kernel_f32<32, E>, &biconvex_admm_kernel_f32<64, E>); }
