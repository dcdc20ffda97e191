// The fp32 instantiations of the batched centroidal ADMM for TWO feet: biconvex_admm_f32.hip's kernels with E = 2, built with the same
// flags as that file (no SLP vectoriser: the reasons are in its header; bunmpc_amd/build.py).
#include "biconvex_kernels.h"
#include <algorithm>
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"      // (biconvex_admm_kernel_f32)

}  // namespace

hipError_t launch_biconvex_admm_f32_e2(const BatchArgs &a, int lpp, unsigned grid, size_t lds, hipStream_t stream) {
    return launch_f32<2>(a, lpp, grid, lds, stream);
}

int biconvex_admm_f32_e2_scratch_bytes() { return f32_scratch_bytes<2>(); }

}  // namespace bunmpc
