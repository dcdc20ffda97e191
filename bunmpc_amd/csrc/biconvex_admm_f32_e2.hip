// The fp32 instantiations of the batched centroidal ADMM for TWO feet: biconvex_admm_f32.hip's kernels with E = 2, built with the same
// flags as that file (no SLP vectoriser: the reasons are in its header; bunmpc_amd/build.py).
#include "biconvex_kernels.h"
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"

}  // namespace

const AdmmUnit &admm_unit_f32_e2() {
    static const AdmmUnit unit = {launch_f32<2>, scratch_bytes<F32Insts<2>>};
    return unit;
}

}  // namespace bunmpc
