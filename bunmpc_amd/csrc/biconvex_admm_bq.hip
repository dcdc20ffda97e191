// The block-cost instantiations of the batched centroidal ADMM for FOUR feet: per-knot block-diagonal Q in set_cost_x / set_cost_f
// (the reference's ProblemData takes a sparse matrix: problem.cpp:31-56; a block per knot is the class that keeps the solve
// matrix-free with one knot per lane).  The body is biconvex_admm_body.h with BQ, the kernel and its launch are in
// biconvex_admm_inst.h; a translation unit of their own so that the units build in parallel and the other kernels' code objects stay
// what they were (bunmpc_amd/build.py).
#include "biconvex_kernels.h"
#include <mutex>

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_inst.h"

}  // namespace

const AdmmUnit &admm_unit_bq_e4() {
    static const AdmmUnit unit = {launch_shape<kBlocks, 4>, scratch_bytes<ShapeInsts<kBlocks, 4>>};
    return unit;
}

}  // namespace bunmpc
