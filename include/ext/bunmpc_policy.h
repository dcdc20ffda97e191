/* bunmpc_policy.h -- the policy network on the device, inference only: a further header of libbunmpc_hip.so, bound by
 * bunmpc_amd/_lib_policy.py.
 *
 * The network is GoalConditionedPolicyNet of ISL/examples/iterative_algorithm/networks.py (ISL = iterative_supervised_learning):
 * Linear(in, hidden), optional BatchNorm1d, ReLU, n_layers times, then Linear(hidden, out), evaluated in fp32 in eval() mode.  It is what
 * the rows of bunmpc_dataset.h's batch are made for (dagger_modified.py:205-226) and what every rollout of simulation.py calls once per
 * simulated millisecond (:1699-1731).  Training and gradients are not here.
 *
 * The header stands alone: it includes nothing.  Status codes and bmpc_last_error() are those of bunmpc.h.  `long` is 64 bits wide
 * (LP64); every stride is in elements.
 *
 * THE FUNCTION, for one input row (bunmpc_amd/policy.py::host_forward is the same text in numpy, and the two agree in every bit):
 *
 *  a. Input.  Either x [n][in] fp64 with a row stride, or state [n][43] and goal [n][w_goal] fp64, 43 + w_goal == in, each with its own
 *     row stride, concatenated state first.  With the second form and mean, std [in] given: v = (v - mean[k]) / std[k] in fp64, IEEE
 *     subtract and divide, unfused, no guard against std == 0.  Then every value is rounded to the nearest-even fp32.
 *  b. Layer l of n_layers + 1, K inputs a[], N outputs: acc = b[j]; for k = 0 .. Kp - 1 ascending: acc = fmaf(W[j][k], a[k], acc) in fp32
 *     with subnormals kept, where Kp is K rounded up to a multiple of BMPC_POLICY_PAD and W[j][k] = a[k] = +0 for k >= K.  (The padding
 *     can do one thing only: an acc of -0 becomes +0.)
 *  c. With batch_norm, on every layer but the last: acc = fmaf(acc, s[j], t[j]), s = gamma / sqrt(running_var + eps) and
 *     t = beta - running_mean * s computed in fp64 by the packer from the fp32 arrays and rounded once to fp32.
 *  d. On every layer but the last: a'[j] = acc <= 0 ? +0 : acc (a NaN stays a NaN).
 *  e. Outputs, each optional (NULL: not written), all fp64 and unfused:
 *       action [n][out]  the fp32 result widened;
 *       tau [n][12]      from q [n][19] and v [n][18] (strided: a [q | v] buffer is used in place with both strides 37), a = action:
 *                          BMPC_POLICY_TORQUE     (out 12)  tau[i] = a[i]
 *                          BMPC_POLICY_PD_TARGET  (out 12)  tau[i] = kp * (a[i] - q[7 + i]) - kd * v[6 + i]
 *                          BMPC_POLICY_STRUCTURED (out 36)  tau[i] = (a[i] + kp * (a[12 + i] - q[7 + i])) + kd * (a[24 + i] - v[6 + i])
 *                        (simulation.py:1714-1731);
 *       err [n]          e = 0; for j ascending: e = e + |(double)a[j] - (double)(float)label[j]| against label [n][out] fp64 with a row
 *                        stride: the row's summand of nn.L1Loss(reduction='sum'); the caller reduces.
 *     No row's result depends on another row. */
#ifndef BUNMPC_POLICY_H
#define BUNMPC_POLICY_H
#ifdef __cplusplus
extern "C" {
#endif

#define BMPC_POLICY_STATE_WIDTH 43
#define BMPC_POLICY_Q_WIDTH 19
#define BMPC_POLICY_V_WIDTH 18
#define BMPC_POLICY_TAU_WIDTH 12
#define BMPC_POLICY_MAX_LAYERS 8      /* hidden layers */
#define BMPC_POLICY_MAX_WIDTH 512     /* of the input and of a hidden layer */
#define BMPC_POLICY_MAX_OUT 64
#define BMPC_POLICY_PAD 16            /* K and N of a layer in the packed image are rounded up to this */
#define BMPC_POLICY_TORQUE 0
#define BMPC_POLICY_PD_TARGET 1
#define BMPC_POLICY_STRUCTURED 2

typedef struct {
    int n_in, n_hidden, n_layers, n_out;   /* 1..512, 1..512, 1..8 hidden layers, 1..64 */
    int batch_norm;                   /* != 0: step c */
    long packed_bytes;                /* bmpc_policy_packed_bytes(...) of the five fields above */
    const void *packed;               /* the packed image: host memory for the packer, device memory (16-byte aligned) for the forward pass */
} bmpc_policy_net_t;
int bmpc_policy_net_struct_size(void);      /* sizeof(bmpc_policy_net_t), to catch binding drift */

/* rows of one workgroup of the forward kernel: the sizes n at which its paths change are multiples of this */
int bmpc_policy_tile(void);

/* bytes of the packed image; -1 where a size is out of range */
long bmpc_policy_packed_bytes(int n_in, int n_hidden, int n_layers, int n_out, int batch_norm);

/* the network's arrays in host memory, fp32, as torch's state_dict holds them: layer l = 0 .. n_layers (the last one is the output layer) */
typedef struct {
    const void *W[9], *b[9];          /* W[l]: [N_l][K_l] row-major fp32, b[l]: [N_l] fp32 */
    const void *gamma[8], *beta[8], *running_mean[8], *running_var[8];   /* [hidden] fp32 each, looked at with batch_norm only */
    double eps;                       /* BatchNorm1d's eps */
} bmpc_policy_weights_t;
int bmpc_policy_weights_struct_size(void);

/* Host code.  Writes the image to net->packed (host memory, net->packed_bytes bytes): per layer, in fp32,
 *   W   [Np / 16][Kp / 16][64][4]: entry (jt, kq, lane, i) is W[16 jt + lane % 16][16 kq + 4 i + lane / 16], +0 outside [N][K];
 *   b   [Np];  and with batch_norm on every layer but the last  s [Np], t [Np]  (step c), +0 beyond N.
 * One lane of the kernel reads 16 consecutive bytes of it per four MFMAs, a wave 1 KiB. */
int bmpc_policy_pack_host(const bmpc_policy_net_t *net, const bmpc_policy_weights_t *weights);

typedef struct {
    long n;                           /* rows, 0 <= n < 2^31; 0 launches nothing */
    /* input, form 1 */
    const double *x;                  /* [n] rows of n_in; NULL: form 2 */
    long x_stride;                    /* >= n_in */
    /* input, form 2 */
    const double *state, *goal;       /* rows of 43 and of w_goal = n_in - 43 */
    long state_stride, goal_stride;   /* >= 43, >= w_goal */
    const double *mean, *std;         /* [n_in] device, state columns first; neither or both; form 2 only */
    /* outputs and what they need */
    double *action;                   /* [n][n_out] dense */
    double *tau;                      /* [n][12] dense */
    int action_type;                  /* BMPC_POLICY_TORQUE, _PD_TARGET (n_out 12), _STRUCTURED (n_out 36) */
    const double *q, *v;              /* rows of 19 and of 18; not looked at for BMPC_POLICY_TORQUE */
    long q_stride, v_stride;          /* >= 19, >= 18 */
    double kp, kd;
    double *err;                      /* [n] */
    const double *label;              /* rows of n_out, required with err */
    long label_stride;                /* >= n_out */
} bmpc_policy_rows_t;
int bmpc_policy_rows_struct_size(void);

/* One kernel launch on hip_stream (NULL: the default stream), asynchronous, no host synchronisation.  A workgroup takes
 * bmpc_policy_tile() rows; the activations stay in LDS from the first layer to the last; HBM sees the input rows once and the outputs
 * once.  The products run on the fp32 matrix cores (v_mfma_f32_16x16x4_f32), whose result is the fmaf chain of step b. */
int bmpc_policy_forward_device(const bmpc_policy_net_t *net, const bmpc_policy_rows_t *rows, void *hip_stream);

/* Every call refuses with BMPC_BAD_ARG and a message naming the field, before anything is launched or written: a NULL descriptor,
 * n_in, n_hidden outside [1, 512], n_layers outside [1, 8], n_out outside [1, 64], packed_bytes other than the query's answer, a NULL
 * or misaligned packed image, a NULL weight array, n outside [0, 2^31), both or neither input form, 43 + w_goal != n_in with w_goal < 1,
 * a stride below its width, one of mean / std without the other or either beside x, tau with an unknown action_type or an n_out other
 * than the type's, tau without q or v where the type reads them, err without label. */

#ifdef __cplusplus
}
#endif
#endif
