// The block-cost instantiations of the batched centroidal ADMM for TWO feet (bipeds): see biconvex_admm_bq.hip.
#include "biconvex_kernels.h"

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"
#include "biconvex_admm_body.h"
#include "biconvex_admm_bq_inst.h"

}  // namespace

hipError_t launch_admm_bq_e2(const BatchArgs &a, const BlockArgs &q, int lpp, hipStream_t stream) { return launch_admm_bq<2>(a, q, lpp, stream); }
int admm_bq_scratch_bytes_e2() { return admm_bq_scratch_bytes<2>(); }

}  // namespace bunmpc
