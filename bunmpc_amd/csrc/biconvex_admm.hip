// Batched centroidal bi-convex ADMM (force-QP / motion-QP alternation by projected
// FISTA) for gfx950 (MI355X, CDNA4).  One launch = B independent
// BiConvexMP::optimize(x_init, num_iters) calls, every ADMM and FISTA iteration
// inside the kernel.
//
// Reference behaviour restated (paths under iterative_supervised_learning/):
//   src/motion_planner/biconvex.cpp:80-120   ADMM loop, P update, exits
//   src/motion_planner/biconvex.cpp:27-78    create_bound_constraints / create_cost_X / _F
//   src/dynamics/centroidal.cpp:57-84        A_x, b_x (force step)
//   src/dynamics/centroidal.cpp:6-37,86-127  A_f, b_f (motion step)
//   include/dynamics/centroidal.hpp:22-27    x_init rows
//   src/solvers/problem.cpp:31-56            gradient / objective difference
//   src/solvers/fista.cpp:6-70               FISTA, backtracking, "SoC" projection
//
// MI355X mapping (this is not how the reference is organised):
//   * one knot per lane, one problem per LPP-lane segment of a wave64
//     (LPP = 16/32/64 >= H+1), so a wave carries 4/2/1 problems; 64-thread
//     workgroups, B*LPP/64 of them -- one barrier (momentum table), no inter-workgroup traffic;
//   * matrix-free operators: lane t applies its own 6x12 block of A_x and its own
//     block-row / block-column of the block-bidiagonal A_f; the explicit Hessian
//     2(Q + rho A^T A) the reference rebuilds every ADMM iteration never exists;
//   * knot t <-> t+-1 coupling of A_f through DPP wave shifts (v_mov_b32_dpp
//     wave_shr/wave_shl), the three per-iteration scalars (||d||^2, g.d, objective
//     difference) through a DPP butterfly + v_permlane16/32_swap -- all lanes of a
//     segment end up with bit-identical sums, so every accept / exit decision is
//     segment-uniform without a broadcast;
//   * the affine images A y + bPk are carried through the momentum step by
//     linearity, so an iteration costs one A and one A^T application instead of the
//     reference's three sparse mat-vecs;
//   * fp64 arithmetic (R = double; MFMA has no advantage over VALU for fp64 on gfx950 and the
//     blocks are 6x12 / 9x9 sparse), FISTA state in VGPRs; between phases X / F / P of a problem
//     rest in LDS (each lane touches only its own knot's blocks), so HBM sees the inputs once and
//     the results once;
//   * R = float is the mixed-precision variant (BASELINE config 3): iterates, operators and
//     projections in fp32, while every decision the algorithm takes -- the backtracking test,
//     both exit tests, the dynamics violation -- is reduced and compared in fp64.  HBM keeps fp64.
//
// This file is every centroidal unit: it is compiled once per cost shape, precision and foot count, with three defines that say
// which (bunmpc_amd/build.py lists the units and gives each its flags), and instantiates that unit's kernels alone.  Which kernel a
// batch gets, and the launch, are in biconvex_launch.hip.
#include "biconvex_kernels.h"
#include <mutex>

#if !defined(ADMM_UNIT_SHAPE) || !defined(ADMM_UNIT_PRECISION) || !defined(ADMM_UNIT_FEET)
#error "biconvex_admm.hip is compiled per unit: -DADMM_UNIT_SHAPE=<a CostShape> -DADMM_UNIT_PRECISION=<0 | 1> -DADMM_UNIT_FEET=<2 | 4>"
#endif

namespace bunmpc {
namespace {

#include "biconvex_lanes.h"

#include "biconvex_admm_body.h"

#include "biconvex_admm_inst.h"

static_assert(unit_is_built(ADMM_UNIT_SHAPE, ADMM_UNIT_PRECISION, ADMM_UNIT_FEET), "no row of kShapes allows this unit");

// a unit's instantiations and its launch (biconvex_admm_inst.h)
template <CostShape SHAPE, int PRECISION, int E>
struct Unit {
    using Insts = ShapeInsts<SHAPE, E>;
    static constexpr auto launch = &launch_shape<SHAPE, E>;
};
template <int E>
struct Unit<kDiag, 0, E> {
    using Insts = AdmmInsts<E>;
    static constexpr auto launch = &launch_admm<E>;
};
template <int E>
struct Unit<kDiag, 1, E> {
    using Insts = F32Insts<E>;
    static constexpr auto launch = &launch_f32<E>;
};
using ThisUnit = Unit<ADMM_UNIT_SHAPE, ADMM_UNIT_PRECISION, ADMM_UNIT_FEET>;

}  // namespace

template <>
const AdmmUnit &admm_unit_of<ADMM_UNIT_SHAPE, ADMM_UNIT_PRECISION, ADMM_UNIT_FEET>() {
    static const AdmmUnit unit = {ThisUnit::launch, scratch_bytes<ThisUnit::Insts>, loop_constants_resident_waves<ThisUnit::Insts>, foot_pair_phases<ThisUnit::Insts>};
    return unit;
}

}  // namespace bunmpc
