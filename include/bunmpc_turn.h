/* bunmpc_turn.h -- turning commands (w_des, a desired yaw rate per problem) through the device-side plan builders: the third header
 * of libbunmpc_hip.so.
 *
 * What SoloMpcGaitGen.optimize(q, v, t, v_des, w_des) does with w_des != 0 (ISL/examples/mpc/abstract_cyclic_gen.py; ISL =
 * iterative_supervised_learning), for B problems at once on top of bmpc_plan_batch_device / bmpc_wb_plan_batch_device and their
 * terrain variants (bunmpc.h).  bunmpc_amd/cyclic_gen.py is the host mirror the tests hold these calls to, problem by problem.
 *
 * The header stands alone: it includes nothing and refers to the structs of bunmpc.h as const void * (bunmpc_amd/_lib.py reads it
 * with the reader of bunmpc.h).  Status codes and bmpc_last_error() are those of bunmpc.h.
 *
 * Per problem b, with w = w_des[b]; the branch is on w != 0 exactly, as in the reference (a NaN takes the turning branch and gives a
 * non-finite plan; nothing is indexed by w):
 *   ori_des   q[3:7] if w != 0, else the identity quaternion                                                        (:636-639)
 *   amom      yaw = atan2(R[1,0], R[0,0]) of R(ori_des), R_des = Rz(yaw), amom = log3(R_des R_q^T); w == 0: log3(R_q^T), what
 *             bmpc_wb_plan_batch_device computes                                                        (:585-591, 616-627)
 *   costs     X_ter[6:9] = amom, X_nom[6::9] = amom[0] ori_correction[0], X_nom[7::9] = amom[1] ori_correction[1]   (:594-600)
 *             w == 0: X_nom[8::9] = amom[2] ori_correction[2]
 *             w != 0: X_nom[8::9] = X_ter[8] = yaw_inertia * w                                                      (:602-607)
 *             yaw_inertia = rdata.Ycrb[1].inertia[2, 2] of the nominal configuration (:48-49), computed once on the host
 *             (cyclic_gen.composite_inertia_base); (I [0, 0, w])[2] is that product exactly for a finite I
 *   steps     the centrifugal term cross(0.5 sqrt(z / g) v_des, [0, 0, w]) of every new location (:285-286, 347-348) is in the plan
 *             kernel of bunmpc.h already; it now sees the caller's w.
 * Everything else -- v_des rotation, rounding, the first-knot dt rule, IK task blocks -- is the plain call's. */
#ifndef BUNMPC_TURN_H
#define BUNMPC_TURN_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const double *w_des;     /* device, [B]: the whole-body call's yaw-rate commands; NULL in the centroidal-level call */
    double yaw_inertia;      /* finite and > 0 */
} bmpc_turn_t;
int bmpc_turn_struct_size(void);             /* sizeof(bmpc_turn_t), to catch binding drift */

/* bmpc_plan_batch_device (terrain == NULL) or bmpc_plan_batch_terrain_device with the yaw-momentum reference: the yaw rate is the
 * plan's own w_des [B], as in those calls, and turn->w_des must be NULL; X_nom[6::9], X_nom[7::9] and X_ter[6:8] come from the plan's
 * amom as there.  plan: a bmpc_plan_batch_t *; terrain: a bmpc_terrain_t * or NULL (flat ground; normals is then not looked at).
 * turn == NULL is the plain call (or the terrain call), bit for bit. */
int bmpc_plan_batch_turn_device(const void *plan, const void *terrain, double *normals, const bmpc_turn_t *turn, void *hip_stream);

/* bmpc_wb_plan_batch_device (terrain == NULL) or bmpc_wb_plan_batch_terrain_device with turning commands: turn->w_des [B] is
 * required and is copied into the struct's w_des intermediate, from where the plan kernels read it.  wb_plan: a
 * bmpc_wb_plan_batch_t *.  turn == NULL is the plain call (or the terrain call), bit for bit; so is every problem with w == 0.
 *
 * Both are asynchronous on hip_stream (NULL: the default stream), allocate nothing and do not synchronise.  BMPC_BAD_ARG, returned
 * before anything is written or launched, with a message naming the field: yaw_inertia not finite or <= 0, a NULL turn->w_des in the
 * whole-body call, a non-NULL turn->w_des in the centroidal-level call, and everything the plain calls refuse. */
int bmpc_wb_plan_batch_turn_device(const void *wb_plan, const void *terrain, double *normals, const bmpc_turn_t *turn, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
