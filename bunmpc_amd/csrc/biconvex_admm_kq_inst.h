// The neighbour-knot-cost kernels of the batched centroidal ADMM (biconvex_admm_body.h: KQ) and their launch, templated on the number of
// feet E.  Included inside the anonymous namespace of one translation unit per foot count (after biconvex_lanes.h and
// biconvex_admm_body.h):
//   biconvex_admm_kq.hip     E = 4        biconvex_admm_kq_e2.hip    E = 2
// built with the flags of biconvex_admm.hip / biconvex_admm_e2.hip (bunmpc_amd/build.py).  Raw form, fp64, one wave per SIMD: beside
// what the diagonal kernel holds a phase keeps the coupling weights of its knot's two pairs (2 x 3E or 2 x 9 values) and, over a FISTA
// iteration, its two neighbours' y.
#pragma once

template <int LPP, int E, bool HASQF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void biconvex_admm_kq_kernel(const BatchArgs a, const BandArgs q) {
    admm_body<double, LPP, E, true, HASQF, false, false, 1, false, true>(a, BlockArgs{}, q);
}

template <int LPP, int E>
hipError_t launch_kq_lpp(const BatchArgs &a, const BandArgs &q, hipStream_t stream) {
    const int per_wave = 64 / LPP;
    const unsigned grid = (unsigned)((a.B + per_wave - 1) / per_wave);
    const size_t lds = sizeof(double) * (kLdsZeros + per_wave * ((size_t)kSegLds + (size_t)knot_lds(E) * (size_t)(a.H + 1)));
    if (a.qf) hipLaunchKernelGGL((biconvex_admm_kq_kernel<LPP, E, true>), dim3(grid), dim3(64), lds, stream, a, q);
    else hipLaunchKernelGGL((biconvex_admm_kq_kernel<LPP, E, false>), dim3(grid), dim3(64), lds, stream, a, q);
    return hipGetLastError();
}

template <int E>
hipError_t launch_admm_kq(const BatchArgs &a, const BandArgs &q, int lpp, hipStream_t stream) {
    if (!a.raw || a.precision != 0 || a.H + 1 > lpp) return hipErrorInvalidValue;
    switch (lpp) {
        case 16: return launch_kq_lpp<16, E>(a, q, stream);
        case 21: return launch_kq_lpp<21, E>(a, q, stream);
        case 32: return launch_kq_lpp<32, E>(a, q, stream);
        case 64: return launch_kq_lpp<64, E>(a, q, stream);
        default: return hipErrorInvalidValue;
    }
}

// private-segment (scratch) bytes per lane, the largest over the neighbour-knot-cost kernels of one foot count
template <int E>
int admm_kq_scratch_bytes() {
    size_t worst = 0;
    for (const void *k : {reinterpret_cast<const void *>(&biconvex_admm_kq_kernel<16, E, false>), reinterpret_cast<const void *>(&biconvex_admm_kq_kernel<16, E, true>),
                          reinterpret_cast<const void *>(&biconvex_admm_kq_kernel<21, E, false>), reinterpret_cast<const void *>(&biconvex_admm_kq_kernel<21, E, true>),
                          reinterpret_cast<const void *>(&biconvex_admm_kq_kernel<32, E, false>), reinterpret_cast<const void *>(&biconvex_admm_kq_kernel<32, E, true>),
                          reinterpret_cast<const void *>(&biconvex_admm_kq_kernel<64, E, false>), reinterpret_cast<const void *>(&biconvex_admm_kq_kernel<64, E, true>)}) {
        hipFuncAttributes at;
        if (hipFuncGetAttributes(&at, k) != hipSuccess) return -1;
        worst = at.localSizeBytes > worst ? at.localSizeBytes : worst;
    }
    return (int)worst;
}
