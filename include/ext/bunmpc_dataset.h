/* bunmpc_dataset.h -- the data set of the trainers on the device: a further header of libbunmpc_hip.so, bound by
 * bunmpc_amd/_lib_dataset.py.
 *
 * What ISL/examples/iterative_algorithm/database.py keeps on the host (ISL = iterative_supervised_learning) -- a ring buffer of rows
 * states (43), vc_goals (5), cc_goals (3 n_eff goal_horizon), actions (12), the input statistics (calc_input_mean_std, :187-213) and the
 * normalised __getitem__ that a DataLoader collates (:53-83) -- for buffers in HBM, appended to by the generator's device tensors
 * without a host synchronisation.  bunmpc_amd/dataset.py stays the host class and the way to disk; tests/dataset_np.py is the numpy
 * restatement these calls are held to.
 *
 * The header stands alone: it includes nothing.  Status codes and bmpc_last_error() are those of bunmpc.h.  `long` is 64 bits wide
 * (LP64); every element offset is one.
 *
 * The ring, as Database.append's row-by-row loop leaves it (:121-143): row j of n appended rows goes to slot
 * (start + length + j) % limit of the start and length before the call; where n > limit only the last `limit` rows are written; then
 * length = min(limit, length + n) and start moves on by what overflowed.  Statistics and batches address buffer rows [0, length), buffer
 * order, as the reference does. */
#ifndef BUNMPC_DATASET_H
#define BUNMPC_DATASET_H
#ifdef __cplusplus
extern "C" {
#endif

#define BMPC_DS_STATE_WIDTH 43
#define BMPC_DS_VC_WIDTH 5
#define BMPC_DS_ACTION_WIDTH 12
#define BMPC_DS_MAX_CC_WIDTH 768      /* 3 n_eff goal_horizon at n_eff = 4, goal_horizon = 64 */
#define BMPC_DS_GOAL_VC 0
#define BMPC_DS_GOAL_CC 1
#define BMPC_DS_HEADER_LONGS 4        /* start, length, rows appended by the last append call, 0 */
#define BMPC_DS_MAX_PROBLEMS 16777216 /* B of one append call */

typedef struct {
    long limit;                       /* rows of every buffer, 1 <= limit < 2^31 */
    int w_states, w_vc, w_cc, w_actions;   /* 43, 5, 3 n_eff goal_horizon (0: no cc_goals group), 12 */
    int max_problems;                 /* the largest B an append call may bring: sizes the scratch */
    /* device, caller-allocated */
    double *states, *vc_goals, *cc_goals, *actions;   /* [limit][width]; cc_goals is not looked at when w_cc == 0 */
    long *header;                     /* [BMPC_DS_HEADER_LONGS]; zero it once, then the calls alone maintain it */
    void *scratch;                    /* bmpc_dataset_scratch_bytes(limit, w_cc, max_problems) bytes, 16-byte aligned */
    long scratch_bytes;
} bmpc_dataset_t;
int bmpc_dataset_struct_size(void);   /* sizeof(bmpc_dataset_t), to catch binding drift */

/* bytes of scratch a data set of these sizes needs (per-problem counts and offsets of an append, per-workgroup partial sums of the
 * statistics); -1 where limit, w_cc or max_problems is out of range */
long bmpc_dataset_scratch_bytes(long limit, int w_cc, int max_problems);

/* the rows one append call brings: B problems of R rows each, device arrays [B][R][width] */
typedef struct {
    int B, R;                         /* 0 <= B <= max_problems, 1 <= R, B R < 2^31 */
    int w_states, w_vc, w_cc, w_actions;   /* widths of the arrays below: the data set's */
    int drop_nonfinite;               /* != 0: a problem whose kept rows hold a NaN or an infinity in any given group brings no row */
    const double *states, *actions;   /* required */
    const double *vc_goals, *cc_goals;/* one may be NULL: that group's slots keep their contents; both NULL is refused */
    const int *rows;                  /* [B] leading rows of problem b that go in, clipped to [0, R]; NULL: R */
    const int *keep;                  /* [B] 0: nothing of problem b goes in; NULL: all */
} bmpc_dataset_rows_t;
int bmpc_dataset_rows_struct_size(void);

/* Appends the kept rows, problems ascending and rows ascending within a problem.  Asynchronous on hip_stream (NULL: the default stream):
 * kernels are enqueued -- per-problem counts, an exclusive prefix over B, one scatter of every given group, the header's update, each a
 * kernel of its own, so stream order is the only synchronisation -- and the call returns; start, length and the wrap are read and written
 * on the device, nothing is copied to the host, and consecutive calls on one stream compose. */
int bmpc_dataset_append_device(const bmpc_dataset_t *ds, const bmpc_dataset_rows_t *rows, void *hip_stream);

/* Per column of states and of cc_goals over buffer rows [0, length): mean and population standard deviation as numpy defines them, in
 * two passes (the mean; the square root of the mean squared deviation from it), IEEE sqrt and division; length == 0 gives NaN.  The sums
 * are trees of a fixed shape -- per-workgroup partials stored plainly, summed in a fixed order by a following kernel, no floating-point
 * atomics: the same contents give the same bits.  states_mean, states_std [43]; cc_mean, cc_std [w_cc], not looked at when w_cc == 0.
 * (The vc_goals statistics are the reference's constants 0.0 and 1.0: nothing to compute.)  Asynchronous, no host synchronisation. */
int bmpc_dataset_moments_device(const bmpc_dataset_t *ds, double *states_mean, double *states_std, double *cc_mean, double *cc_std,
                                void *hip_stream);

/* The batch view: x[i] = [state | goal], y[i] = action of buffer row index[i], dense: x [n][43 + goal width], y [n][12]. */
typedef struct {
    long n;                           /* 0 <= n < 2^31 */
    const long *index;                /* [n] device; outside [0, length): that row of x and y is NaN, nothing is read */
    int goal_type;                    /* BMPC_DS_GOAL_VC or BMPC_DS_GOAL_CC */
    int normalise;                    /* != 0: (v - mean) / std, IEEE subtract and divide; vc goals go through (v - 0.0) / 1.0 */
    const double *states_mean, *states_std;   /* [43] device, required when normalise */
    const double *goal_mean, *goal_std;       /* [w_cc] device, required when normalise and goal_type is cc; not looked at otherwise */
    double *x, *y;
} bmpc_dataset_batch_t;
int bmpc_dataset_batch_struct_size(void);
int bmpc_dataset_batch_device(const bmpc_dataset_t *ds, const bmpc_dataset_batch_t *batch, void *hip_stream);

/* Every call refuses with BMPC_BAD_ARG and a message naming the field, before anything is launched or written: a NULL descriptor or
 * required pointer, limit outside [1, 2^31), widths other than 43, 5, 12 and a multiple of 3 in [0, 768], max_problems outside
 * [1, 2^24], scratch_bytes below the query's answer, B, R or n out of range, B above max_problems, widths of the rows that differ from
 * the data set's, both goal arrays NULL, cc_goals given to (or goal_type cc asked of) a data set without that group. */

#ifdef __cplusplus
}
#endif
#endif
