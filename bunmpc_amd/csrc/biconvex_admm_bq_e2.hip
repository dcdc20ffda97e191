// The block-cost instantiations of the batched centroidal ADMM for TWO feet: biconvex_admm_bq.hip's kernels with E = 2, built with the
// same flags (bunmpc_amd/build.py).
#include "biconvex_kernels.h"
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"

}  // namespace

const AdmmUnit &admm_unit_bq_e2() {
    static const AdmmUnit unit = {launch_shape<kBlocks, 2>, scratch_bytes<ShapeInsts<kBlocks, 2>>};
    return unit;
}

}  // namespace bunmpc
