/* bunmpc_goals.h -- contact-conditioned goals (`cc_goals`) on the device: the second header of libbunmpc_hip.so.
 *
 * What the reference computes where a contact-conditioned policy is deployed (ISL/examples/iterative_algorithm/simulation.py:999-1006;
 * ISL = iterative_supervised_learning): a Raibert contact plan over the whole episode, its contact switches and the per-foot
 * schedule (contact_planner.py:35-59, 61-256; utils.py:104-120), the estimated CoM (utils.py:187-219) and the goal rows
 * (utils.py:36-102), for B problems at once and without leaving HBM.  Planner-derived goals only: the goals that the data collection
 * builds from contacts measured in the simulator (simulation.py:563-568) are not computed here.
 *
 * The header stands alone: it includes nothing and declares its own structs (bunmpc_amd/_lib.py reads it with the reader of
 * bunmpc.h).  Status codes and bmpc_last_error() are those of bunmpc.h; `model` is a bmpc_model_t * of bmpc_model_create.
 *
 * Per problem b, in the reference's order:
 *   plan      H_cp = bmpc_cc_goal_plan_knots(...) knots, every one gait_dt long, from round(com, 3)[0:2], com[2], round(feet0, 3),
 *             the yaw-rotated hip offsets hip_off, v_des as given (no rotation) and w_des; knot i >= 1 at round(t0 + i gait_dt, 3);
 *   switches  knot i >= 1, foot in contact at i and not at i - 1: [t0 / sim_dt + i gait_dt / sim_dt, x, y, 1e-3], appended to
 *             that foot's events: schedule [B][4][max_events][4], zeros after a foot's counts[b][foot] events;
 *   goals     N_total = all feet's events together; end_time = int(min(episode_length + 1, min_foot max(schedule row, zero padded to
 *             N_total))); start_step = int(t0 / sim_dt); one row per t in [start_step, end_time); slot (gh, foot) of the row is
 *             [schedule[foot][k][0] - t, com_row[0:2] - schedule[foot][k][1:3]], k = ee_contact_index(t, foot) + gh, where an index
 *             from the foot's count up to N_total - 1 reads zeros, as in the reference's array.
 *             com_row = com_rows[b][t - start_step], or with com_rows == NULL the estimated CoM
 *             round(com, 3)[0:2] + (t - start_step) sim_dt v_des[0:2].
 *   rows[b]   the number of goal rows, at most max_rows; goals [B][max_rows][3 * 4 * goal_horizon], zeros from row rows[b] on.
 *   status[b] 0, or one of the bits below: where the reference raises, this writes no row and says why. */
#ifndef BUNMPC_GOALS_H
#define BUNMPC_GOALS_H
#ifdef __cplusplus
extern "C" {
#endif

#define BMPC_CC_FEW_SWITCHES 1        /* fewer than two switches in the plan: no schedule (utils.py:114); rows = 0 */
#define BMPC_CC_START_AFTER_END 2     /* start_step >= end_time: no row (utils.py:57) */
#define BMPC_CC_PAST_SCHEDULE 4       /* a slot's k >= N_total (utils.py:66 raises): rows = the leading rows free of it */
#define BMPC_CC_EVENTS_OVERFLOW 8     /* N_total > max_events: schedule holds each foot's first max_events events; rows = 0 */

typedef struct {
    double gait_period, gait_dt, gait_horizon;
    double stance_percent[4], phase_offset[4];
} bmpc_cc_gait_t;

typedef struct {
    int B, n_eff, episode_length, goal_horizon;   /* n_eff: 4 */
    int max_rows, max_events, n_knots, reserved_;  /* n_knots: H_cp, must equal bmpc_cc_goal_plan_knots(...) */
    double sim_dt;                                 /* 0.001 in the reference (contact_planner.py:14) */
    bmpc_cc_gait_t gait;
    const double *t0;                  /* [B] start time in seconds (sim_t) */
    const double *com;                 /* [B][3] centre of mass, unrounded */
    const double *feet0;               /* [B][4][3] current foot positions, unrounded */
    const double *hip_off;             /* [B][4][2] (R_yaw offsets[j])[0:2] (contact_planner.py:94-124, :188) */
    const double *v_des;               /* [B][3] */
    const double *w_des;               /* [B] */
    const double *com_rows;            /* [B][max_rows][3] or NULL: the estimated CoM */
    double *goals;                     /* [B][max_rows][12 goal_horizon] */
    int *rows, *status;                /* [B] */
    double *schedule;                  /* [B][4][max_events][4] */
    int *counts;                       /* [B][4] events of each foot (all of them, also past max_events) */
    double *cnt_plan, *swing_time;     /* [B][n_knots][4][4], [B][n_knots][4], or both NULL: the plan is not wanted */
} bmpc_cc_goal_batch_t;

/* int(20.0 * episode_length * sim_dt * gait_horizon * gait_period / gait_dt) (contact_planner.py:130); -1 where that is not a
 * finite number in [0, 2^30].  Pure: no GPU, no library state. */
int bmpc_cc_goal_plan_knots(int episode_length, double sim_dt, double gait_horizon, double gait_period, double gait_dt);
int bmpc_cc_goal_batch_struct_size(void);
int bmpc_cc_goal_wb_batch_struct_size(void);

/* Asynchronous on hip_stream (NULL: the default stream).  BMPC_BAD_ARG, before anything is launched, with a message that names the
 * limit: B outside [0, 2^20], episode_length outside [1, 2^20], max_rows outside [1, 2^20], goal_horizon < 1 or > 64, n_eff != 4,
 * max_events < 2 or > 2^16, n_knots != bmpc_cc_goal_plan_knots(...) or < 1 or > 2^20, an array of more than 2^40 bytes, sim_dt or
 * a gait number that is not finite and > 0 (stance percents in (0, 1], phase offsets finite), a required pointer that is NULL,
 * exactly one of cnt_plan / swing_time. */
int bmpc_cc_goal_batch_device(const bmpc_cc_goal_batch_t *d, void *hip_stream);

/* The same from whole-body states x = [q, v]: kinematics on the device (CoM, feet, hips), then
 * offsets[j] = round(hip_j - com, 3), y widened by +0.04 / -0.04 / +0.04 / -0.04, R(q)^T offsets[j] with the full base rotation,
 * and hip_off[j] = (R_yaw offsets[j])[0:2] with the yaw of matrixToRpy (contact_planner.py:80-124).  g.com, g.feet0 and g.hip_off are
 * ignored: the front end writes com, feet0, hips and hip_off below (caller-allocated, device) and the batch call reads them. */
typedef struct {
    const void *model;                 /* bmpc_model_t * */
    int foot_frame[4], hip_frame[4];   /* frame indices of eff_names and hip_names */
    const double *x;                   /* [B][37] */
    double *com, *feet0, *hips, *hip_off;   /* [B][3], [B][4][3], [B][4][3], [B][4][2] */
    bmpc_cc_goal_batch_t g;
} bmpc_cc_goal_wb_batch_t;
int bmpc_cc_goal_wb_batch_device(const bmpc_cc_goal_wb_batch_t *d, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
