// The instantiations of the batched centroidal ADMM with the Euclidean cone projection, TWO feet: biconvex_admm_cone.hip's kernels with
// E = 2, built with the same flags (bunmpc_amd/build.py).
#include "biconvex_kernels.h"
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"

}  // namespace

const AdmmUnit &admm_unit_cone_e2() {
    static const AdmmUnit unit = {launch_shape<kCone, 2>, scratch_bytes<ShapeInsts<kCone, 2>>};
    return unit;
}

}  // namespace bunmpc
