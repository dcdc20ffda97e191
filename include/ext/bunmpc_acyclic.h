/* bunmpc_acyclic.h -- acyclic motions (jumps, rearing: plans given as time tables) through the device-side data path: a further
 * header of libbunmpc_hip.so, bound by bunmpc_amd/_lib_acyclic.py.
 *
 * What SoloAcyclicGen.create_contact_plan / create_costs and the zero-order-hold expansion of SoloAcyclicGen.optimize do per MPC call
 * (ISL/examples/mpc/abstract_acyclic_gen.py:74-296, 331-345; ISL = iterative_supervised_learning), for B problems at once that share
 * ONE motion table.  bunmpc_amd/acyclic_gen.py is the host mirror these calls are held to, array by array and bit by bit
 * (tests/acyclic_np.py packs what the mirror hands its solver objects into the arrays below).
 *
 * The header stands alone: it includes nothing and refers to the model of bunmpc.h as const void *.  Status codes and
 * bmpc_last_error() are those of bunmpc.h.
 *
 * Per problem b at time t = t[b] of a motion started at t0[b], H = n_col knots, dt_arr the table's knot lengths:
 *   two time walks   contact table:  ft = round3(t - dt_arr[0] - t0);  ft += round3(dt_arr[i])      -- no rounding after the sum (:76-80)
 *                    every other:    ft = t - dt_arr[0] - t0;  ft = round3(ft + dt_arr[min(i, H - 1)])                  (:127-131 ...)
 *                    so one knot can sit in different phases of different tables.
 *   a table look-up  ft < the last row's end time: the first row with start <= ft < end, or, where none matches (a negative motion
 *                    time, a gap), zeros / no cost at that node; otherwise (past the end, and a NaN time, which matches no interval)
 *                    the last row is held; X_nom takes X_ter there, and so does the terminal reference when that knot is the last.
 *   dt               dt[0] = dt_arr[0] - round2(remainder(t, dt_arr[0])) on the ABSOLUTE t, 0 becomes dt_arr[0] (:110-115); dt_ik is
 *                    dt_arr as it stands: the IK stage does not see the first-knot rule (:225).
 *   centroidal state x_init = [com, vcom, hg.angular] of x, by the kernel of bmpc_ik_centroidal_state_device (what the solve itself
 *                    starts from); X_nom knot 0 = x_init (:185).
 *   IK task blocks   the layout of bmpc_ik_batch_t.tasks.  Frame tasks of a running node: contacts first (flag == 1: weight cnt_wt,
 *                    reference cnt_plan[i][j][1:4]), then the swing window's feet with weight > 0 (:193-222); a node that needs more
 *                    than four keeps the first four in that order and sets BMPC_ACY_FRAME_SLOTS in status[b].  CoM and momentum
 *                    weights cent_wt at every node (their references are filled by bmpc_kinodyn_solve_batch_device).
 *   regularisation   node i <= H: state scale in tasks[31], state_w / x_reg rows from the state tables; the phase comes from
 *                    state_scale[k][1:3], the end time is state_end = state_reg[-1][-1] (:229-250).  Control: running nodes carry
 *                    the weight ctrl_wt[k][0] -- the first entry of the weight VECTOR, as the reference passes it (:262, 277) --, the
 *                    terminal block carries ctrl_scale[k][0].  A node without the cost: weight 0, zero weight vectors, and the neutral
 *                    reference (unit quaternion) in x_reg.
 * Every entry of every output is written on every call.  No table content becomes an index: the row counts are the struct's ints. */
#ifndef BUNMPC_ACYCLIC_H
#define BUNMPC_ACYCLIC_H
#ifdef __cplusplus
extern "C" {
#endif

#define BMPC_ACY_FRAME_SLOTS 1      /* status bit: a node needed more than four frame tasks */
#define BMPC_ACY_MAX_PHASES 16

typedef struct {
    int B, n_col;
    int n_cnt, n_x, n_b, n_sw, n_s, n_c;   /* rows of the tables below: each in [1, BMPC_ACY_MAX_PHASES]; n_sw may be 0 (a scalar swing_wt) */
    int foot_frame[4];                     /* frame indices of the end effectors (eff_names) in the model */
    const void *model;                     /* a bmpc_model_t * */
    double cnt_wt, cent_wt[2];             /* finite */
    double state_end;                      /* state_reg[-1][-1] */
    /* inputs, device */
    const double *x;                       /* [B][37] */
    const double *t, *t0;                  /* [B] */
    /* the motion table, device */
    const double *dt_arr;                  /* [n_col] */
    const double *tab_cnt_plan;            /* [n_cnt][4][6]: flag, position, start, end */
    const double *tab_X_nom;               /* [n_x][11] */
    const double *tab_X_ter;               /* [9] */
    const double *tab_bounds;              /* [n_b][8] */
    const double *tab_swing_wt;            /* [n_sw][4][6]: weight, position, start, end; not looked at when n_sw == 0 */
    const double *tab_state_reg;           /* [n_s][37] */
    const double *tab_state_wt;            /* [n_s][36] */
    const double *tab_state_scale;         /* [n_s][3]: scale, start, end */
    const double *tab_ctrl_wt;             /* [n_c][18] */
    const double *tab_ctrl_scale;          /* [n_c][3] */
    /* outputs, device, caller-allocated */
    double *cnt_plan;                      /* [B][H][4][4] */
    double *dt, *dt_ik;                    /* [B][H] */
    double *x_init;                        /* [B][9] */
    double *X_nom;                         /* [B][9H] */
    double *X_ter;                         /* [B][9] */
    double *bounds;                        /* [B][H][6] */
    double *ik_tasks;                      /* [B][H+1][33] */
    double *state_w, *x_reg, *ctrl_w;      /* [B][H+1][36], [B][H+1][37], [B][H][18] */
    int *status;                           /* [B] */
} bmpc_acyclic_plan_t;
int bmpc_acyclic_plan_struct_size(void);     /* sizeof(bmpc_acyclic_plan_t), to catch binding drift */

/* Asynchronous on hip_stream (NULL: the default stream), allocates nothing and does not synchronise.  BMPC_BAD_ARG, returned before
 * anything is written or launched, with a message naming the field: a NULL descriptor, model, input, table or output (tab_swing_wt
 * may be NULL when n_sw == 0), B < 0, n_col outside [1, 255], a row count outside [1, 16] (n_sw: [0, 16]), a foot frame outside the
 * model, a cnt_wt, cent_wt or state_end that is not finite (state_end may be +inf).  The tables are device memory: not looked at. */
int bmpc_acyclic_plan_batch_device(const bmpc_acyclic_plan_t *d, void *hip_stream);

/* The 1 kHz plan of SoloAcyclicGen.optimize (:331-345), a zero-order hold: out[b] = vstack_{i < size} tile(knots[b][i], int(dt[b][i] / step)).
 * knots [B][n_knots][width], dt [B][dt_stride] (first `size` entries used, size <= n_knots), out [B][max_rows][width];
 * rows [B] = rows written for each problem: min(the sum, max_rows).  Rows of out past that are set to 0.
 * The fields of bmpc_interp_batch_t (bunmpc.h), whose call interpolates between the knots instead. */
typedef struct {
    int B, n_knots, width, size, max_rows, dt_stride;
    double step;
    const double *knots, *dt;
    double *out;
    int *rows;
} bmpc_hold_batch_t;
int bmpc_hold_batch_struct_size(void);       /* sizeof(bmpc_hold_batch_t) */
/* Asynchronous, allocates nothing, does not synchronise.  BMPC_BAD_ARG naming the field: a NULL descriptor or array, B < 0, n_knots,
 * width, size or max_rows < 1, size > n_knots, dt_stride < size, step not finite and > 0, more than 2^38 output entries. */
int bmpc_hold_batch_device(const bmpc_hold_batch_t *d, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
