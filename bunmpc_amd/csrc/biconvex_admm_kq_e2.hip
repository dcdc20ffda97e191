// The instantiations of the batched centroidal ADMM for costs that couple neighbouring knots, TWO feet: a Q in set_cost_x /
// set_cost_f that is block-tridiagonal over the knots with diagonal off-diagonal blocks -- force-rate and momentum-rate terms D'R D
// (the reference's ProblemData takes a sparse matrix: problem.cpp:31-56).  The body is biconvex_admm_body.h with KQ; a translation unit
// of their own so that the units build in parallel and the other kernels' code objects stay what they were (bunmpc_amd/build.py).
#include "biconvex_kernels.h"

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_kq_inst.h"

}  // namespace

hipError_t launch_admm_kq_e2(const BatchArgs &a, const BandArgs &q, int lpp, hipStream_t stream) { return launch_admm_kq<2>(a, q, lpp, stream); }
int admm_kq_scratch_bytes_e2() { return admm_kq_scratch_bytes<2>(); }

}  // namespace bunmpc
