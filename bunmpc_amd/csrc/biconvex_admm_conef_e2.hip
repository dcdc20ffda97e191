// The instantiations of the batched centroidal ADMM with the Euclidean cone projection about per-contact surface normals, TWO feet:
// biconvex_admm_conef.hip's kernels with E = 2, built with the same flags (bunmpc_amd/build.py).
#include "biconvex_kernels.h"
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"

}  // namespace

const AdmmUnit &admm_unit_conef_e2() {
    static const AdmmUnit unit = {launch_shape<kConeFrame, 2>, scratch_bytes<ShapeInsts<kConeFrame, 2>>};
    return unit;
}

}  // namespace bunmpc
