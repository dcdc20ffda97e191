// The kernels of the batched centroidal ADMM and their launches, templated on the number of feet E.  Included inside the anonymous
// namespace of one translation unit per cost shape, precision and foot count (after biconvex_lanes.h and biconvex_admm_body.h), each
// of which instantiates its own launch and exports it as one AdmmUnit (biconvex_kernels.h):
//   biconvex_admm.hip        fp64, E = 4   launch_admm        biconvex_admm_f32.hip      fp32, E = 4   launch_f32
//   biconvex_admm_e2.hip     fp64, E = 2                      biconvex_admm_f32_e2.hip   fp32, E = 2
//   biconvex_admm_bq.hip     blocks, E = 4   launch_bq        biconvex_admm_kq.hip       band, E = 4   launch_kq
//   biconvex_admm_bq_e2.hip  blocks, E = 2                    biconvex_admm_kq_e2.hip    band, E = 2
//   biconvex_admm_cone.hip   Euclidean cone projection, E = 4   launch_cone
//   biconvex_admm_cone_e2.hip                           E = 2
//   biconvex_admm_conef.hip  ... about per-contact normals, E = 4   launch_conef
//   biconvex_admm_conef_e2.hip                             E = 2
// so that every unit is built with its own flags (bunmpc_amd/build.py), the units build in parallel and one feature's kernels cannot
// disturb another's code object.  Which kernel a batch gets is decided once, for every unit, by plan_launch (biconvex_admm.hip).
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

// Per-knot block costs (biconvex_admm_body.h: BQ).  Raw form, fp64, one wave per SIMD: the force phase holds the knot's 3E x 3E block
// (78 values at four feet) beside what the diagonal kernel holds, the motion phase its 9 x 9 block (45).
template <int LPP, int E, bool HASQF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void biconvex_admm_bq_kernel(const BatchArgs a, const BlockArgs q) {
    admm_body<double, LPP, E, true, HASQF, false, false, 1, true>(a, q);
}
// Costs between neighbouring knots (biconvex_admm_body.h: KQ).  Raw form, fp64, one wave per SIMD: beside what the diagonal kernel holds
// a phase keeps the coupling weights of its knot's two pairs (2 x 3E or 2 x 9 values) and, over a FISTA iteration, its two neighbours' y.
template <int LPP, int E, bool HASQF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void biconvex_admm_kq_kernel(const BatchArgs a, const BandArgs q) {
    admm_body<double, LPP, E, true, HASQF, false, false, 1, false, true>(a, BlockArgs{}, q);
}
// The Euclidean cone projection with per-foot friction coefficients (biconvex_admm_body.h: CONE).  Both forms, fp64, one wave per SIMD:
// beside what the diagonal kernel holds a lane keeps its knot's E coefficients over the whole solve.
template <int LPP, int E, bool RAW, bool HASQF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void biconvex_admm_cone_kernel(const BatchArgs a, const ConeArgs c) {
    admm_body<double, LPP, E, RAW, HASQF, false, false, 1, false, false, true>(a, BlockArgs{}, c);
}
// ... about per-contact surface normals (biconvex_admm_body.h: FRAME): the cone kernel, and a lane keeps its knot's 3E normal components
// beside the E coefficients.
template <int LPP, int E, bool RAW, bool HASQF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void biconvex_admm_conef_kernel(const BatchArgs a, const ConeFrameArgs c) {
    admm_body<double, LPP, E, RAW, HASQF, false, false, 1, false, false, true, true>(a, BlockArgs{}, c);
}

// The one switch over the lanes per problem: f(std::integral_constant<int, LPP>) of the plan's lpp.  A launch names the values its unit
// instantiates with `if constexpr` and refuses the others.
template <typename F>
hipError_t with_lpp(int lpp, F &&f) {
    switch (lpp) {
        case 16: return f(std::integral_constant<int, 16>{});
        case 21: return f(std::integral_constant<int, 21>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        case 192: return f(std::integral_constant<int, 192>{});
        case 256: return f(std::integral_constant<int, 256>{});
        default: return hipErrorInvalidValue;
    }
}
// a kernel of 64 / LPP problems per wave over the batch, with its arguments
template <int LPP, int E, typename K, typename... A>
hipError_t launch_segments(K kernel, size_t elem, const BatchArgs &a, hipStream_t stream, const A &...args) {
    hipLaunchKernelGGL(kernel, dim3(launch_grid(a.B, 64 / LPP)), dim3(64), launch_lds_bytes(elem, 64 / LPP, E, a.H), stream, a, args...);
    return hipGetLastError();
}

template <int LPP, int E, bool RAW, bool HASQF>
hipError_t launch(const BatchArgs &a, bool two_per_simd, hipStream_t stream) {
    if (two_per_simd) return launch_segments<LPP, E>(biconvex_admm_kernel<double, LPP, E, RAW, HASQF, 2>, sizeof(double), a, stream);
    return launch_segments<LPP, E>(biconvex_admm_kernel<double, LPP, E, RAW, HASQF, 1>, sizeof(double), a, stream);
}

template <int E, int WAVES, bool RAW, bool HASQF, int WPE>
hipError_t launch_wg(const BatchArgs &a, hipStream_t stream) {
    // more than the 64 KB a kernel may take without asking, from 209 knots on: raised once per device and instantiation
    static std::mutex lock;
    static bool raised[16] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return hipErrorInvalidDevice;
    {
        std::lock_guard<std::mutex> hold(lock);
        if (!raised[dev]) {
            const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&biconvex_admm_wg_kernel<E, WAVES, RAW, HASQF, WPE>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
            if (attr != hipSuccess) return attr;
            raised[dev] = true;
        }
    }
    hipLaunchKernelGGL((biconvex_admm_wg_kernel<E, WAVES, RAW, HASQF, WPE>), dim3(launch_grid(a.B, 1)), dim3(64 * WAVES), launch_lds_bytes(sizeof(double), 1, E, a.H, (size_t)WAVES * 40), stream, a);
    return hipGetLastError();
}
template <int E, int WAVES, int WPE>
hipError_t launch_wg_form(const BatchArgs &a, hipStream_t stream) {
    if (a.precision != 0) return hipErrorInvalidValue;      // (fp64 only)
    if (!a.raw) return launch_wg<E, WAVES, false, false, WPE>(a, stream);
    return a.qf ? launch_wg<E, WAVES, true, true, WPE>(a, stream) : launch_wg<E, WAVES, true, false, WPE>(a, stream);
}

// the launch plan_launch decided on, fp64 with diagonal costs: batch kernel, workgroup kernel, or the persistent grid of the
// work-stealing kernel (a.queue: its device counter, set by the caller)
template <int E>
hipError_t launch_admm(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream) {
    if (a.precision != 0) return hipErrorInvalidValue;
    if (l.steal) {
        const size_t lds = launch_lds_bytes(sizeof(double), 3, E, a.H);
        if (l.w2) hipLaunchKernelGGL((biconvex_admm_steal_kernel<E, 2>), dim3((unsigned)l.steal_waves), dim3(64), lds, stream, a);
        else hipLaunchKernelGGL((biconvex_admm_steal_kernel<E, 1>), dim3((unsigned)l.steal_waves), dim3(64), lds, stream, a);
        return hipGetLastError();
    }
    return with_lpp(l.lpp, [&](auto lanes) {
        constexpr int LPP = decltype(lanes)::value;
        if constexpr (LPP > 64) return l.w2 ? launch_wg_form<E, LPP / 64, 2>(a, stream) : launch_wg_form<E, LPP / 64, 1>(a, stream);
        else if (!a.raw) return launch<LPP, E, false, false>(a, l.w2, stream);
        else return a.qf ? launch<LPP, E, true, true>(a, l.w2, stream) : launch<LPP, E, true, false>(a, l.w2, stream);
    });
}
// ... fp32 (the units built without the SLP vectoriser): harness form, 16 / 32 / 64 lanes per problem
template <int E>
hipError_t launch_f32(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream) {
    if (a.precision != 1 || a.raw) return hipErrorInvalidValue;
    return with_lpp(l.lpp, [&](auto lanes) {
        constexpr int LPP = decltype(lanes)::value;
        if constexpr (LPP == 16 || LPP == 32 || LPP == 64) return launch_segments<LPP, E>(biconvex_admm_kernel_f32<LPP, E>, sizeof(float), a, stream);
        else return hipErrorInvalidValue;
    });
}
// ... block costs and costs between neighbouring knots: raw form, fp64, at most 64 lanes per problem
template <int E>
hipError_t launch_bq(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream) {
    if (!a.raw || a.precision != 0 || a.H + 1 > l.lpp) return hipErrorInvalidValue;
    const BlockArgs q = {l.cost.x, l.cost.f, l.cost.sx, l.cost.sf};
    return with_lpp(l.lpp, [&](auto lanes) {
        constexpr int LPP = decltype(lanes)::value;
        if constexpr (LPP > 64) return hipErrorInvalidValue;
        else return a.qf ? launch_segments<LPP, E>(biconvex_admm_bq_kernel<LPP, E, true>, sizeof(double), a, stream, q)
                         : launch_segments<LPP, E>(biconvex_admm_bq_kernel<LPP, E, false>, sizeof(double), a, stream, q);
    });
}
template <int E>
hipError_t launch_kq(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream) {
    if (!a.raw || a.precision != 0 || a.H + 1 > l.lpp) return hipErrorInvalidValue;
    const BandArgs q = {l.cost.x, l.cost.f, l.cost.sx, l.cost.sf};
    return with_lpp(l.lpp, [&](auto lanes) {
        constexpr int LPP = decltype(lanes)::value;
        if constexpr (LPP > 64) return hipErrorInvalidValue;
        else return a.qf ? launch_segments<LPP, E>(biconvex_admm_kq_kernel<LPP, E, true>, sizeof(double), a, stream, q)
                         : launch_segments<LPP, E>(biconvex_admm_kq_kernel<LPP, E, false>, sizeof(double), a, stream, q);
    });
}
// ... the Euclidean cone projection: either form, fp64, at most 64 lanes per problem
template <int E>
hipError_t launch_cone(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream) {
    if (a.precision != 0 || a.H + 1 > l.lpp) return hipErrorInvalidValue;
    const ConeArgs c = {l.cost.f, l.cost.sf};
    return with_lpp(l.lpp, [&](auto lanes) {
        constexpr int LPP = decltype(lanes)::value;
        if constexpr (LPP > 64) return hipErrorInvalidValue;
        else if (!a.raw) return launch_segments<LPP, E>(biconvex_admm_cone_kernel<LPP, E, false, false>, sizeof(double), a, stream, c);
        else return a.qf ? launch_segments<LPP, E>(biconvex_admm_cone_kernel<LPP, E, true, true>, sizeof(double), a, stream, c)
                         : launch_segments<LPP, E>(biconvex_admm_cone_kernel<LPP, E, true, false>, sizeof(double), a, stream, c);
    });
}
// ... the same about per-contact normals (l.cost.x, never null here: without normals the C-ABI takes the cone kernel)
template <int E>
hipError_t launch_conef(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream) {
    if (a.precision != 0 || a.H + 1 > l.lpp || !l.cost.x) return hipErrorInvalidValue;
    const ConeFrameArgs c = {l.cost.f, l.cost.sf, l.cost.x, l.cost.sx};
    return with_lpp(l.lpp, [&](auto lanes) {
        constexpr int LPP = decltype(lanes)::value;
        if constexpr (LPP > 64) return hipErrorInvalidValue;
        else if (!a.raw) return launch_segments<LPP, E>(biconvex_admm_conef_kernel<LPP, E, false, false>, sizeof(double), a, stream, c);
        else return a.qf ? launch_segments<LPP, E>(biconvex_admm_conef_kernel<LPP, E, true, true>, sizeof(double), a, stream, c)
                         : launch_segments<LPP, E>(biconvex_admm_conef_kernel<LPP, E, true, false>, sizeof(double), a, stream, c);
    });
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
template <int E>
int f32_scratch_bytes() { return max_scratch_bytes(&biconvex_admm_kernel_f32<16, E>, &biconvex_admm_kernel_f32<32, E>, &biconvex_admm_kernel_f32<64, E>); }
template <int E>
int bq_scratch_bytes() {
    return max_scratch_bytes(&biconvex_admm_bq_kernel<16, E, false>, &biconvex_admm_bq_kernel<16, E, true>, &biconvex_admm_bq_kernel<21, E, false>, &biconvex_admm_bq_kernel<21, E, true>,
                             &biconvex_admm_bq_kernel<32, E, false>, &biconvex_admm_bq_kernel<32, E, true>, &biconvex_admm_bq_kernel<64, E, false>, &biconvex_admm_bq_kernel<64, E, true>);
}
template <int E>
int kq_scratch_bytes() {
    return max_scratch_bytes(&biconvex_admm_kq_kernel<16, E, false>, &biconvex_admm_kq_kernel<16, E, true>, &biconvex_admm_kq_kernel<21, E, false>, &biconvex_admm_kq_kernel<21, E, true>,
                             &biconvex_admm_kq_kernel<32, E, false>, &biconvex_admm_kq_kernel<32, E, true>, &biconvex_admm_kq_kernel<64, E, false>, &biconvex_admm_kq_kernel<64, E, true>);
}
template <int E, int LPP>
int cone_lpp_scratch_bytes() {
    return max_scratch_bytes(&biconvex_admm_cone_kernel<LPP, E, false, false>, &biconvex_admm_cone_kernel<LPP, E, true, false>, &biconvex_admm_cone_kernel<LPP, E, true, true>);
}
template <int E>
int cone_scratch_bytes() {
    int worst = 0;
    for (int s : {cone_lpp_scratch_bytes<E, 16>(), cone_lpp_scratch_bytes<E, 21>(), cone_lpp_scratch_bytes<E, 32>(), cone_lpp_scratch_bytes<E, 64>()}) {
        if (s < 0) return -1;
        worst = s > worst ? s : worst;
    }
    return worst;
}
template <int E, int LPP>
int conef_lpp_scratch_bytes() {
    return max_scratch_bytes(&biconvex_admm_conef_kernel<LPP, E, false, false>, &biconvex_admm_conef_kernel<LPP, E, true, false>, &biconvex_admm_conef_kernel<LPP, E, true, true>);
}
template <int E>
int conef_scratch_bytes() {
    int worst = 0;
    for (int s : {conef_lpp_scratch_bytes<E, 16>(), conef_lpp_scratch_bytes<E, 21>(), conef_lpp_scratch_bytes<E, 32>(), conef_lpp_scratch_bytes<E, 64>()}) {
        if (s < 0) return -1;
        worst = s > worst ? s : worst;
    }
    return worst;
}
