// The instantiations of the batched centroidal ADMM with the Euclidean cone projection about per-contact surface normals, FOUR feet
// (bmpc_contact_frame_t: the cone's axis is the contact's unit normal, not world z).  The body is biconvex_admm_body.h with CONE and
// FRAME, the kernel and its launch are in biconvex_admm_inst.h; a translation unit of their own, as the cone kernels have: the units
// build in parallel and every other kernel's code object stays what it was (bunmpc_amd/build.py).
#include "biconvex_kernels.h"
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"

}  // namespace

const AdmmUnit &admm_unit_conef_e4() {
    static const AdmmUnit unit = {launch_shape<kConeFrame, 4>, scratch_bytes<ShapeInsts<kConeFrame, 4>>};
    return unit;
}

}  // namespace bunmpc
