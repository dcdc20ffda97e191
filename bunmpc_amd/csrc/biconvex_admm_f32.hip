// The fp32 instantiations of the batched centroidal ADMM kernel (BASELINE config 3: fp32 iterates, operators and projections;
// every decision of the algorithm reduced and compared in fp64 -- see biconvex_admm.hip for the mapping and the reference lines).
//
// A translation unit of its own because it is built with -fno-slp-vectorize (bunmpc_amd/build.py): hipcc's SLP vectoriser packs
// pairs of fp32 operations into v_pk_mul/fma/add_f32, which need their operands in adjacent register pairs -- 47 v_mov_b32 per
// backtracking step to put them there, duplicated copies of the broadcast constants, 284-307 registers, and so 40-60 values
// spilled to scratch memory under the cap of 256 that two waves per SIMD need (345 MB of HBM traffic per launch against 75 MB of
// inputs and results; profiles/r02_pmc_hbm_cfg3.txt).  Without the packing the body takes 200-212 registers: no scratch, and
// Go2 H = 40, B = 4096 goes 7.09 -> 6.02 ms.  (The fp64 kernels are ~0.5 % faster WITH the vectoriser, hence the split.)
#include "biconvex_kernels.h"
#include <algorithm>
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"      // (biconvex_admm_kernel_f32)

}  // namespace

hipError_t launch_biconvex_admm_f32(const BatchArgs &a, int lpp, unsigned grid, size_t lds, hipStream_t stream) {
    return launch_f32<4>(a, lpp, grid, lds, stream);
}

// private-segment (scratch) bytes per lane of the fp32 instantiations, the largest of the three: 0 is the point of this file
int biconvex_admm_f32_scratch_bytes() { return f32_scratch_bytes<4>(); }

}  // namespace bunmpc
