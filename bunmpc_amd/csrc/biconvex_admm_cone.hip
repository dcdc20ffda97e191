// The instantiations of the batched centroidal ADMM with the Euclidean projection onto the friction cone and per-foot friction
// coefficients, FOUR feet (bmpc_cone_t; the reference's own "SoC" step, fista.cpp:52-70, is what every other unit restates).  The body is
// biconvex_admm_body.h with CONE, the kernel and its launch are in biconvex_admm_inst.h; a translation unit of their own so that the
// units build in parallel and the other kernels' code objects stay what they were (bunmpc_amd/build.py).
#include "biconvex_kernels.h"
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"

}  // namespace

const AdmmUnit &admm_unit_cone_e4() {
    static const AdmmUnit unit = {launch_shape<kCone, 4>, scratch_bytes<ShapeInsts<kCone, 4>>};
    return unit;
}

}  // namespace bunmpc
