// The kernels of the batched centroidal ADMM and their launches, templated on the number of feet E.  Included inside the anonymous
// namespace of biconvex_admm.hip (after biconvex_lanes.h and biconvex_admm_body.h), which is compiled once per cost shape, precision
// and foot count and exports that unit's launch and list of instantiations as one AdmmUnit (biconvex_kernels.h: admm_unit_of):
//   kDiag, fp64                      launch_admm, AdmmInsts
//   kDiag, fp32                      launch_f32, F32Insts
//   every other shape (fp64)         launch_shape<SHAPE, E>, ShapeInsts<SHAPE, E>
// bunmpc_amd/build.py lists the units and gives each its flags.  Which kernel a batch gets is decided once, for every unit, by
// plan_launch (biconvex_launch.hip).
// A new cost shape is: its CostShape value with its row of kShapes and its struct in ShapeExtra (biconvex_kernels.h), its kernel
// template below with its lines in shape_kernel / shape_extra, its name in bunmpc_amd/build.py, and its `if constexpr` code in the
// body.
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
    admm_body<AdmmCfg<R, LPP, E, RAW, HASQF, false, WPE == 2>>(a);
}
// ... and the WPE = 2 build of the 32-lane harness-form kernel whose certified loops keep x_k in registers and 18 phase constants in LDS
// (biconvex_admm_body.h: CLDS; 17 .. 21 knots at four feet: loop_constants_fit)
template <int E>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void biconvex_admm_clds_kernel(const BatchArgs a) {
    admm_body<AdmmCfg<double, 32, E, false, false, false, true, 1, kDiag, true>>(a);
}
// ... and that build in workgroups of EIGHT waves, two per SIMD of a CU, each with its own two problems and its own LDS area: the waves
// that share a SIMD see each other and keep level (biconvex_admm_body.h: MATES)
template <int E>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void biconvex_admm_clds_mates_kernel(const BatchArgs a) {
    admm_body<AdmmCfg<double, 32, E, false, false, false, true, 1, kDiag, true, true>>(a);
}
// horizons of 64 .. 255 knots: one problem per workgroup of WAVES waves (biconvex_admm_body.h: WAVES)
template <int E, int WAVES, bool RAW, bool HASQF, int WPE>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void biconvex_admm_wg_kernel(const BatchArgs a) {
    admm_body<AdmmCfg<double, 64, E, RAW, HASQF, false, WPE == 2, WAVES>>(a);
}
// the work-stealing variant (biconvex_admm_body.h: STEAL): three problems per wave, harness form, fp64
template <int E, int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void biconvex_admm_steal_kernel(const BatchArgs a) {
    admm_body<AdmmCfg<double, 21, E, false, false, true, WPE == 2>>(a);
}
// fp32: TWO waves per SIMD -- this latency-bound loop gains a second wave to issue from while the first waits (one wave per SIMD:
// 9.0 ms).  Instantiated only in the fp32 units (bunmpc_amd/build.py explains their flags).
template <int LPP, int E>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void biconvex_admm_kernel_f32(const BatchArgs a) {
    admm_body<AdmmCfg<float, LPP, E, false, false>>(a);
}

// Per-knot block costs (biconvex_admm_body.h: BQ).  Raw form, fp64, one wave per SIMD: the force phase holds the knot's 3E x 3E block
// (78 values at four feet) beside what the diagonal kernel holds, the motion phase its 9 x 9 block (45).
template <int LPP, int E, bool HASQF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void biconvex_admm_bq_kernel(const BatchArgs a, const BlockArgs q) {
    admm_body<AdmmCfg<double, LPP, E, true, HASQF, false, false, 1, kBlocks>>(a, q);
}
// Costs between neighbouring knots (biconvex_admm_body.h: KQ).  Raw form, fp64, one wave per SIMD: beside what the diagonal kernel holds
// a phase keeps the coupling weights of its knot's two pairs (2 x 3E or 2 x 9 values) and, over a FISTA iteration, its two neighbours' y.
template <int LPP, int E, bool HASQF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void biconvex_admm_kq_kernel(const BatchArgs a, const BandArgs q) {
    admm_body<AdmmCfg<double, LPP, E, true, HASQF, false, false, 1, kBand>>(a, q);
}
// The Euclidean cone projection with per-foot friction coefficients (biconvex_admm_body.h: CONE).  Both forms, fp64, one wave per SIMD:
// beside what the diagonal kernel holds a lane keeps its knot's E coefficients over the whole solve.
template <int LPP, int E, bool RAW, bool HASQF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void biconvex_admm_cone_kernel(const BatchArgs a, const ConeArgs c) {
    admm_body<AdmmCfg<double, LPP, E, RAW, HASQF, false, false, 1, kCone>>(a, c);
}
// ... about per-contact surface normals (biconvex_admm_body.h: FRAME): the cone kernel, and a lane keeps its knot's 3E normal components
// beside the E coefficients.
template <int LPP, int E, bool RAW, bool HASQF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void biconvex_admm_conef_kernel(const BatchArgs a, const ConeFrameArgs c) {
    admm_body<AdmmCfg<double, LPP, E, RAW, HASQF, false, false, 1, kConeFrame>>(a, c);
}

// One instantiation of a unit: its kernel and the plan that takes it -- lanes per problem (above 64: the workgroup kernel of LPP / 64
// waves), form (0 harness, 1 raw, 2 raw with qf), AdmmLaunch::w2 and ::steal.
template <auto K, int LPP_, int FORM, bool W2 = false, bool STEAL_ = false, bool CLDS_ = false, bool MATES_ = false>
struct Inst {
    static constexpr auto kernel = K;
    static constexpr int LPP = LPP_;
    static constexpr bool STEAL = STEAL_, CLDS = CLDS_, MATES = MATES_;
    static bool planned(const BatchArgs &a, const AdmmLaunch &l) {
        return l.lpp == LPP && l.steal == STEAL && l.w2 == W2 && l.clds == CLDS && l.mates == MATES && (a.raw ? (a.qf ? 2 : 1) : 0) == FORM;
    }
};
// f(std::integral_constant<int, V>) for every V of a list
template <int... V>
using Ints = std::integer_sequence<int, V...>;
template <typename F, int... V>
void each_int(Ints<V...>, F &&f) { (f(std::integral_constant<int, V>{}), ...); }

// The instantiations of each unit, v(Inst<...>{}) for every one: what its launch chooses from and what its scratch query covers.
// fp64, diagonal costs: batch kernel (every lanes-per-problem, form and build), workgroup kernel likewise, work stealing
template <int E_>
struct AdmmInsts {
    static constexpr int E = E_;
    template <typename V>
    static void each(V &&v) {
        each_int(Ints<0, 1, 2>{}, [&](auto form) { each_int(Ints<1, 2>{}, [&](auto wpe) {
            constexpr int FORM = decltype(form)::value, WPE = decltype(wpe)::value;
            each_int(Ints<16, 21, 32, 64>{}, [&](auto lpp) { v(Inst<&biconvex_admm_kernel<double, decltype(lpp)::value, E, (FORM > 0), FORM == 2, WPE>, decltype(lpp)::value, FORM, WPE == 2>{}); });
            each_int(Ints<2, 3, 4>{}, [&](auto waves) { v(Inst<&biconvex_admm_wg_kernel<E, decltype(waves)::value, (FORM > 0), FORM == 2, WPE>, 64 * decltype(waves)::value, FORM, WPE == 2>{}); });
        }); });
        v(Inst<&biconvex_admm_steal_kernel<E, 1>, 21, 0, false, true>{});
        v(Inst<&biconvex_admm_steal_kernel<E, 2>, 21, 0, true, true>{});
        if constexpr (E == 4) v(Inst<&biconvex_admm_clds_kernel<E>, 32, 0, true, false, true>{});
        if constexpr (E == 4) v(Inst<&biconvex_admm_clds_mates_kernel<E>, 32, 0, true, false, true, true>{});
    }
};
// fp32 (the units built without the SLP vectoriser): harness form, 16 / 32 / 64 lanes per problem
template <int E_>
struct F32Insts {
    static constexpr int E = E_;
    template <typename V>
    static void each(V &&v) { each_int(Ints<16, 32, 64>{}, [&](auto lpp) { v(Inst<&biconvex_admm_kernel_f32<decltype(lpp)::value, E>, decltype(lpp)::value, 0>{}); }); }
};
// the other cost shapes: every lanes-per-problem up to 64, the forms the shape is built for (kShapes)
template <CostShape SHAPE, int LPP, int E, bool RAW, bool HASQF>
constexpr auto shape_kernel() {
    if constexpr (SHAPE == kBlocks) return &biconvex_admm_bq_kernel<LPP, E, HASQF>;
    else if constexpr (SHAPE == kBand) return &biconvex_admm_kq_kernel<LPP, E, HASQF>;
    else if constexpr (SHAPE == kCone) return &biconvex_admm_cone_kernel<LPP, E, RAW, HASQF>;
    else return &biconvex_admm_conef_kernel<LPP, E, RAW, HASQF>;
}
template <CostShape SHAPE>
ShapeExtra<SHAPE> shape_extra(const CostArgs &c) {
    if constexpr (SHAPE == kCone) return {c.f, c.sf};
    else if constexpr (SHAPE == kConeFrame) return {c.f, c.sf, c.x, c.sx};
    else return {c.x, c.f, c.sx, c.sf};
}
template <CostShape SHAPE, int E_>
struct ShapeInsts {
    static constexpr int E = E_;
    template <typename V>
    static void each(V &&v) {
        each_int(Ints<16, 21, 32, 64>{}, [&](auto lpp) { each_int(Ints<0, 1, 2>{}, [&](auto form) {
            constexpr int LPP = decltype(lpp)::value, FORM = decltype(form)::value;
            if constexpr (FORM > 0 || !kShapes[SHAPE].raw_only) v(Inst<shape_kernel<SHAPE, LPP, E, (FORM > 0), FORM == 2>(), LPP, FORM>{});
        }); });
    }
};

// Launch one instantiation with the plan's geometry: a kernel of 64 / LPP problems per wave over the batch with the shape's arguments,
// a workgroup per problem, or the persistent grid of the work-stealing kernel
template <typename I, int E, typename... X>
hipError_t launch_inst(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream, const X &...extra) {
    constexpr auto kernel = I::kernel;
    const size_t elem = a.precision == 1 ? sizeof(float) : sizeof(double);
    if constexpr (I::STEAL) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)l.steal_waves), dim3(64), launch_lds_bytes(elem, 3, E, a.H), stream, a);
    } else if constexpr (I::LPP > 64) {
        // more than the 64 KB a kernel may take without asking, from 209 knots on: raised once per device and instantiation
        static std::mutex lock;
        static bool raised[16] = {};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return hipErrorInvalidDevice;
        {
            std::lock_guard<std::mutex> hold(lock);
            if (!raised[dev]) {
                const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
                if (attr != hipSuccess) return attr;
                raised[dev] = true;
            }
        }
        hipLaunchKernelGGL(kernel, dim3(launch_grid(a.B, 1)), dim3(I::LPP), launch_lds_bytes(elem, 1, E, a.H, (size_t)(I::LPP / 64) * 40), stream, a);
    } else if constexpr (I::MATES) {
        // eight waves' areas and the mailbox: more than the 64 KB a kernel may take without asking, raised once per device as above
        if (!loop_constants_fit(E, a.H)) return hipErrorInvalidValue;
        static std::mutex lock;
        static bool raised[16] = {};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return hipErrorInvalidDevice;
        {
            std::lock_guard<std::mutex> hold(lock);
            if (!raised[dev]) {
                const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
                if (attr != hipSuccess) return attr;
                raised[dev] = true;
            }
        }
        hipLaunchKernelGGL(kernel, dim3(launch_grid(a.B, 16)), dim3(512), simd_mates_lds_bytes(E, a.H), stream, a);
    } else if constexpr (I::CLDS) {
        if (!loop_constants_fit(E, a.H)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(kernel, dim3(launch_grid(a.B, 2)), dim3(64), loop_constants_lds_bytes(E, a.H), stream, a);
    } else {
        hipLaunchKernelGGL(kernel, dim3(launch_grid(a.B, 64 / I::LPP)), dim3(64), launch_lds_bytes(elem, 64 / I::LPP, E, a.H), stream, a, extra...);
    }
    return hipGetLastError();
}
// the launch plan_launch decided on, from the unit's instantiations (a.queue: the work-stealing kernel's device counter, set by the caller)
template <typename Insts, typename... X>
hipError_t launch_planned(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream, const X &...extra) {
    hipError_t err = hipErrorInvalidValue;      // (a plan the unit has no kernel for)
    Insts::each([&](auto inst) { if (decltype(inst)::planned(a, l)) err = launch_inst<decltype(inst), Insts::E>(a, l, stream, extra...); });
    return err;
}
template <int E>
hipError_t launch_admm(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream) {
    if (a.precision != 0) return hipErrorInvalidValue;
    return launch_planned<AdmmInsts<E>>(a, l, stream);
}
template <int E>
hipError_t launch_f32(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream) {
    if (a.precision != 1 || a.raw) return hipErrorInvalidValue;
    return launch_planned<F32Insts<E>>(a, l, stream);
}
// ... with the shape's arrays, under the guards of its row of kShapes (kConeFrame: l.cost.x, the normals, is never null here -- without
// normals the C-ABI takes the cone kernel)
template <CostShape SHAPE, int E>
hipError_t launch_shape(const BatchArgs &a, const AdmmLaunch &l, hipStream_t stream) {
    constexpr ShapeInfo s = kShapes[SHAPE];
    if ((s.raw_only && !a.raw) || (s.fp64_only && a.precision != 0) || a.H + 1 > l.lpp || l.lpp > s.max_knots) return hipErrorInvalidValue;
    if (SHAPE == kConeFrame && !l.cost.x) return hipErrorInvalidValue;
    return launch_planned<ShapeInsts<SHAPE, E>>(a, l, stream, shape_extra<SHAPE>(l.cost));
}

// private-segment (scratch) bytes per lane, the largest over the unit's instantiations; -1 on error
template <typename Insts>
int scratch_bytes() {
    long worst = 0;
    Insts::each([&](auto inst) {
        hipFuncAttributes at;
        if (worst < 0 || hipFuncGetAttributes(&at, reinterpret_cast<const void *>(decltype(inst)::kernel)) != hipSuccess) worst = -1;
        else worst = (long)at.localSizeBytes > worst ? (long)at.localSizeBytes : worst;
    });
    return (int)worst;
}

// waves of the unit's loop-constants build that one CU holds at once with the LDS a horizon of H takes (the runtime's occupancy query:
// at k = 21 eight waves fill the CU's LDS to the allocation granule, so the arithmetic alone does not settle it); 0: no such build
template <typename Insts>
int loop_constants_resident_waves(int H) {
    int waves = 0;
    Insts::each([&](auto inst) {
        using I = decltype(inst);
        if constexpr (I::CLDS && !I::MATES) {
            int n = 0;
            const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, I::kernel, 64, loop_constants_lds_bytes(Insts::E, H));
            waves = e == hipSuccess ? n : -1;
        }
    });
    return waves;
}

// (wave, force phase) pairs that the unit's loop-constants build ran two feet per lane on the current device since the last reset
// (biconvex_admm_body.h: g_foot_pair_phases); waits for the device.  0: the unit has no such build, -1 on error
template <typename Insts>
long foot_pair_phases(int reset) {
    bool has = false;
    Insts::each([&](auto inst) { has = has || decltype(inst)::CLDS; });
    if (!has) return 0;
    unsigned long long n = 0;
    const unsigned long long zero = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_foot_pair_phases), sizeof(n)) != hipSuccess) return -1;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_foot_pair_phases), &zero, sizeof(zero)) != hipSuccess) return -1;
    return (long)n;
}
