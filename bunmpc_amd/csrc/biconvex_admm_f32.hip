// The fp32 instantiations of the batched centroidal ADMM kernel (BASELINE config 3: fp32 iterates, operators and projections;
// every decision of the algorithm reduced and compared in fp64 -- see biconvex_admm.hip for the mapping and the reference lines).
//
// A translation unit of its own because it is built with -fno-slp-vectorize (bunmpc_amd/build.py): hipcc's SLP vectoriser packs
// pairs of fp32 operations into v_pk_mul/fma/add_f32, which need their operands in adjacent register pairs -- 47 v_mov_b32 per
// backtracking step to put them there, duplicated copies of the broadcast constants, 284-307 registers, and so 40-60 values
// spilled to scratch memory under the cap of 256 that two waves per SIMD need (345 MB of HBM traffic per launch against 75 MB of
// inputs and results; profiles/r02_pmc_hbm_cfg3.txt).  Without the packing the body takes 200-212 registers: no scratch, and
// Go2 H = 40, B = 4096 goes 7.09 -> 6.02 ms.  (The fp64 kernels are ~0.5 % faster WITH the vectoriser, hence the split.)
// Its scratch bytes (AdmmUnit::scratch_bytes) being 0 is the point of this file.
#include "biconvex_kernels.h"
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"

}  // namespace

const AdmmUnit &admm_unit_f32_e4() {
    static const AdmmUnit unit = {launch_f32<4>, scratch_bytes<F32Insts<4>>};
    return unit;
}

}  // namespace bunmpc
