// The fp64 instantiations of the batched centroidal ADMM for TWO feet (bipeds): the same kernels as biconvex_admm.hip instantiates
// for four (biconvex_admm_inst.h), in a translation unit of their own so that both build in parallel with the same flags
// (bunmpc_amd/build.py).  A knot's LDS record is 33 doubles instead of 39 (knot_lds); plan_launch (biconvex_admm.hip) decides
// which kernel a batch gets, for both foot counts alike.
#include "biconvex_kernels.h"
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"

}  // namespace

const AdmmUnit &admm_unit_e2() {
    static const AdmmUnit unit = {launch_admm<2>, scratch_bytes<AdmmInsts<2>>};
    return unit;
}

}  // namespace bunmpc
