// The instantiations of the batched centroidal ADMM for costs that couple neighbouring knots, FOUR feet: a Q in set_cost_x /
// set_cost_f that is block-tridiagonal over the knots with diagonal off-diagonal blocks -- force-rate and momentum-rate terms D'R D
// (the reference's ProblemData takes a sparse matrix: problem.cpp:31-56).  The body is biconvex_admm_body.h with KQ, the kernel and its
// launch are in biconvex_admm_inst.h; a translation unit of their own so that the units build in parallel and the other kernels' code
// objects stay what they were (bunmpc_amd/build.py).
#include "biconvex_kernels.h"
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"

}  // namespace

const AdmmUnit &admm_unit_kq_e4() {
    static const AdmmUnit unit = {launch_shape<kBand, 4>, scratch_bytes<ShapeInsts<kBand, 4>>};
    return unit;
}

}  // namespace bunmpc
