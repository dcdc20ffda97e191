// The block-cost instantiations of the batched centroidal ADMM for FOUR feet: per-knot block-diagonal Q in set_cost_x / set_cost_f
// (the reference's ProblemData takes a sparse matrix: problem.cpp:31-56; a block per knot is the class that keeps the solve
// matrix-free with one knot per lane).  The body is biconvex_admm_body.h with BQ; a translation unit of their own so that the units
// build in parallel and the other kernels' code objects stay what they were (bunmpc_amd/build.py).
#include "biconvex_kernels.h"

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_bq_inst.h"

}  // namespace

hipError_t launch_admm_bq_e4(const BatchArgs &a, const BlockArgs &q, int lpp, hipStream_t stream) { return launch_admm_bq<4>(a, q, lpp, stream); }
int admm_bq_scratch_bytes_e4() { return admm_bq_scratch_bytes<4>(); }

}  // namespace bunmpc
