// The instantiations of the batched centroidal ADMM for costs that couple neighbouring knots, TWO feet: biconvex_admm_kq.hip's kernels
// with E = 2, built with the same flags (bunmpc_amd/build.py).
#include "biconvex_kernels.h"
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"

}  // namespace

const AdmmUnit &admm_unit_kq_e2() {
    static const AdmmUnit unit = {launch_shape<kBand, 2>, scratch_bytes<ShapeInsts<kBand, 2>>};
    return unit;
}

}  // namespace bunmpc
