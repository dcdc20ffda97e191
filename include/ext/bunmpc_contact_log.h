/* bunmpc_contact_log.h -- measured contact goals: the logged contacts of rollouts turned into cc_goals rows on the device.  A further
 * header of libbunmpc_hip.so, bound by bunmpc_amd/_lib_contact_log.py.
 *
 * What four rollout functions of ISL/examples/iterative_algorithm/simulation.py (ISL = iterative_supervised_learning) do after their
 * simulator has stepped (:537-550 with :563-578, :789-804 with :812-826, :1055-1082, :2026-2049): edge detection on the contact
 * positions logged per step, a per-foot event list, utils.construct_contact_schedule and utils.construct_cc_goal over the MEASURED
 * CoM history, and the number of leading rows of the other three groups that go into the data set.  bunmpc_goals.h builds the
 * planner-derived goals of deployment; this builds the measured goals of data collection.  bunmpc_amd/contact_log.py is the host
 * path; its host_batch() is the numpy twin this call equals bit for bit.
 *
 * The header stands alone: it includes nothing.  Status codes and bmpc_last_error() are those of bunmpc.h.
 *
 * Per episode b, log row r is simulation step o = start_step[b] + r; rows r < n_b = min(T, episode_length - start_step[b]) are used.
 *
 *   new contacts  (:299-314, :437-438, :540-550)  with pre = 0 before row 0, foot j makes a new contact at row r iff
 *                 abs(ee_pos[b][r][j][0]) > 1e-12 and abs(pre[j][0]) <= 1e-12 -- the x component only (a foot in contact at x == 0.0 is
 *                 not in contact; a NaN x is neither a contact nor a cleared predecessor); pre takes the row's values after every
 *                 row.  A new contact is recorded unless o == 0 (the absolute step: an episode with start_step > 0 records the feet
 *                 that stand at its first row).  The event is [o, x, y, z], o as a double, appended to that foot's list.
 *   schedule      (utils.py:104-120)  counts[b][j] = events of foot j over the whole log, N_total their sum; a foot's column is its
 *                 events, by step, then zeros up to N_total.  N_total < 2 is the reference's exception: BMPC_CL_FEW_SWITCHES.
 *   goals         (utils.py:36-102, called with episode_length itself)
 *                 end_time = int(min(episode_length, min_j max(column j over its N_total entries, padding included)));
 *                 one row per t in [start_step, end_time); slot (gh, j) of a row is
 *                     [schedule[j][k][0] - t, com[b][t - start_step][0:2] - schedule[j][k][1:3]],  k = ee_contact_index(t, column j) + gh,
 *                 the scan running over the padding too; k from the foot's count up to N_total - 1 reads zeros; k >= N_total is the
 *                 reference's IndexError: BMPC_CL_PAST_SCHEDULE, rows = the number of leading rows free of it (those rows are
 *                 written).  start_step > end_time is the reference's ValueError: BMPC_CL_START_AFTER_END (start_step == end_time is
 *                 zero rows and no error).
 *   rows[b]       end_time - start_step, clipped to max_rows: the reference's end_time = len(cc_goal_history).
 *   failed states (:189-220, utils.py:7-34; check_failed != 0)  row r fails when r > grace (= gait_period / sim_dt, computed by the caller)
 *                 and q[2] < z_min or q[2] > 2.0 or abs(roll) > fail_angle or abs(pitch) > fail_angle, with (x, y, z, w) = q[3:7],
 *                     roll  = atan2(2 (w x + y z), 1 - 2 (x x + y y)) (180 / pi),
 *                     pitch = asin(clamp(2 (w y - z x), -1, 1)) (180 / pi);
 *                 z_min is 0.05 for jump and bound and 0.1 otherwise.  failed_step[b] = the first failing row r < n_b, or -1; a failed
 *                 episode gets BMPC_CL_FAILED_STATE beside its other bits and rows = 0: the reference returns nothing for it.
 *
 * Every output is defined entry for entry: zeros behind a foot's events up to max_events, zero goal rows from rows[b] on.  schedule
 * and counts are those of the whole log whatever the status.  Under BMPC_CL_EVENTS_OVERFLOW (N_total > max_events) the schedule holds
 * each foot's first max_events events, counts the true numbers, and rows = 0. */
#ifndef BUNMPC_CONTACT_LOG_H
#define BUNMPC_CONTACT_LOG_H
#ifdef __cplusplus
extern "C" {
#endif

#define BMPC_CL_FEW_SWITCHES 1
#define BMPC_CL_START_AFTER_END 2
#define BMPC_CL_PAST_SCHEDULE 4
#define BMPC_CL_EVENTS_OVERFLOW 8
#define BMPC_CL_FAILED_STATE 16

typedef struct {
    int B, T;                         /* episodes, log rows per episode: 0 <= B <= 2^20, 1 <= T <= 2^20 */
    int n_eff;                        /* 4 */
    int goal_horizon;                 /* 1 .. 64 */
    int max_events;                   /* slots of a foot's column, 2 .. 2^16 */
    int max_rows;                     /* goal rows kept per episode, 1 .. T */
    int episode_length;               /* 1 .. 2^20 */
    int check_failed;                 /* != 0: the failed-state test; q is required */
    double z_min, fail_angle, grace;  /* finite, whether or not check_failed is set */
    long s_q;                         /* row stride of q in doubles, >= 19: rows of x = [q, v] (37) can be passed in place */
    /* device, caller-allocated; inputs */
    const int *start_step;            /* [B] int(start_time / sim_dt) */
    const double *ee_pos;             /* [B][T][4][3] */
    const double *com;                /* [B][T][3] */
    const double *q;                  /* [B T] rows of 19 at stride s_q; may be NULL when check_failed == 0 */
    /* outputs */
    double *schedule;                 /* [B][4][max_events][4] */
    int *counts;                      /* [B][4] */
    double *goals;                    /* [B][max_rows][12 goal_horizon] */
    int *rows, *status;               /* [B] */
    int *failed_step;                 /* [B], may be NULL; -1 everywhere when check_failed == 0 */
    double *angles;                   /* [B][T][2] roll and pitch in degrees of every row, may be NULL; written when check_failed != 0 */
} bmpc_contact_log_t;
int bmpc_contact_log_struct_size(void);   /* sizeof(bmpc_contact_log_t), to catch binding drift */

/* Asynchronous on hip_stream (NULL: the default stream); allocates nothing and does not synchronise.  Kernels, each reading what the one
 * before it wrote across a kernel boundary of the stream only: events (one workgroup per episode: the log is read once, in blocks of
 * 64 consecutive rows per wave), failed states (one thread per row, an integer minimum per episode), rows and status (one thread per
 * episode), goals (one thread per (episode, row, slot)).  A call enqueued again on the same buffers gives the same bits.
 *
 * BMPC_BAD_ARG with a message naming the field, before anything is launched or written: a NULL descriptor, B outside [0, 2^20], T or
 * episode_length outside [1, 2^20], max_rows outside [1, T], goal_horizon outside [1, 64], n_eff != 4, max_events outside [2, 2^16], an
 * array (ee_pos, q, goals, schedule) above 2^40 bytes, 2^32 or more goal slots (B max_rows 4 goal_horizon) or, with check_failed, rows (B times T
 * rounded up to 64): more threads than one launch takes, a required pointer NULL, q == NULL with check_failed != 0, s_q below 19
 * where q is given, fail_angle, z_min or grace not finite. */
int bmpc_contact_log_goals_device(const bmpc_contact_log_t *d, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
