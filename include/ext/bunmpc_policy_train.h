/* bunmpc_policy_train.h -- the policy network's training step on the device, and its packed inference image written there: a further
 * header of libbunmpc_hip.so, bound by bunmpc_amd/_lib_policy_train.py.
 *
 * The network and its sizes are those of bunmpc_policy.h (GoalConditionedPolicyNet of ISL/examples/iterative_algorithm/networks.py); the
 * step is one pass of the loop of behavioral_cloning_train.py:123-149: the network in train() mode, nn.L1Loss(), loss.backward(),
 * torch.optim.Adam(lr).step().  The header stands alone: it includes nothing.  Status codes and bmpc_last_error() are those of bunmpc.h.
 * `long` is 64 bits wide (LP64); every stride is in elements.
 *
 * THE FUNCTION (bunmpc_amd/policy_train.py::host_step is the same text in numpy, and the two agree in every bit).  Everything is fp32
 * unless it says fp64; subnormals are kept; `fmaf` is the one-rounding fused multiply-add; +, -, *, /, sqrt are IEEE operations, unfused.
 * "chain over i of t(i)" is: s = +0; for i ascending: s = fmaf(t's two factors, s) (a plain term u is the product u * 1); then
 * s = fmaf(+0, +0, s) where the count is no multiple of BMPC_POLICY_TRAIN_PAD -- the padding of the one reduction rule.  (From a start of
 * +0 a chain never holds -0, so the padding changes a bit in step b alone, whose chain starts from the bias.)  n is the number of rows,
 * L = n_layers, layer l = 0 .. L has K inputs and N outputs, fn = (float)n.
 *
 *  a. Input.  a_0[r][k] = (float)x[r][k], y32[r][j] = (float)y[r][j]: nearest-even.
 *  b. Linear, layer l: z[r][j] = b[j]; for k ascending: z = fmaf(W[j][k], a_l[r][k], z); z = fmaf(+0, +0, z) where K % 16 != 0.
 *  c. BatchNorm1d in train() mode, with batch_norm on every layer but the last, per column j:
 *       mean = (chain over r of z[r][j]) / fn;   d[r] = z[r][j] - mean;   var = (chain over r of d[r] * d[r]) / fn;
 *       invstd = 1 / sqrt(var + (float)eps);     xhat[r][j] = d[r] * invstd;   u[r][j] = fmaf(xhat[r][j], gamma[j], beta[j]);
 *       running_mean[j] = fmaf(0.1f, mean, 0.9f * running_mean[j]);
 *       running_var[j]  = fmaf(0.1f, (var * fn) / (fn - 1), 0.9f * running_var[j]);      0.9f stands for the fp32 difference 1 - 0.1f.
 *     Without batch_norm u = z.
 *  d. ReLU on every layer but the last: a_{l+1}[r][j] = u <= 0 ? +0 : u (a NaN stays a NaN).  The last layer's z is the prediction p.
 *  e. Loss, fp64: e[r] = 0; for j ascending: e[r] = e[r] + |(double)p[r][j] - (double)y32[r][j]| (bunmpc_policy.h's err);
 *     loss = 0; for r ascending: loss = loss + e[r]; loss = loss / (double)(n * n_out).
 *  f. Backward.  c = 1 / (float)(n * n_out); t = p[r][j] - y32[r][j]; dz_L[r][j] = t > 0 ? c : t < 0 ? -c : t == 0 ? +0 : t (NaN).
 *     Per layer l = L .. 0:
 *       db[j]    = chain over r of dz_l[r][j];
 *       dW[j][k] = chain over r of dz_l[r][j] * a_l[r][k];
 *     and for l > 0, towards layer l - 1 whose column is k:
 *       da[r][k] = chain over j of W[j][k] * dz_l[r][j]        (W before this step's update);
 *       du[r][k] = a_l[r][k] <= 0 ? +0 : da[r][k]              (the ReLU's mask u > 0; a NaN activation lets the gradient through);
 *       without batch_norm dz_{l-1} = du; with it
 *         dbeta[k] = chain over r of du[r][k];    dgamma[k] = chain over r of du[r][k] * xhat[r][k];
 *         g = gamma[k] * invstd[k];   mb = dbeta[k] / fn;   mg = dgamma[k] / fn;
 *         dz_{l-1}[r][k] = fmaf(-xhat[r][k], mg, du[r][k] - mb) * g.
 *  g. Adam (torch's single-tensor rule with its defaults: betas 0.9, 0.999, eps 1e-8, no weight decay, no amsgrad), on every element q of
 *     W, b, gamma, beta with gradient gq and moments m, v; b1 = (float)0.9, b2 = (float)0.999, w1 = (float)(1 - 0.9),
 *     w2 = (float)(1 - 0.999) (the fp64 differences rounded), step = (float)(lr / bc1), root = (float)sqrt(bc2) (fp64, rounded once),
 *     bc1 = 1 - 0.9^t and bc2 = 1 - 0.999^t computed by the caller in fp64 for the call's count t = 1, 2, ...:
 *       m = fmaf(w1, gq - m, m);   v = fmaf(w2 * gq, gq, b2 * v);   denom = sqrt(v) / root + (float)1e-8;   q = fmaf(-step, m / denom, q).
 *  Every sum over rows or over outputs is one chain in ascending index owned by one lane: no atomics, no combination whose order depends
 *  on the launch.  The IEEE fp32 sqrt and divide are computed as the fp64 operation rounded once more to fp32, which is the same value
 *  (53 >= 2 * 24 + 2 bits). */
#ifndef BUNMPC_POLICY_TRAIN_H
#define BUNMPC_POLICY_TRAIN_H
#ifdef __cplusplus
extern "C" {
#endif

#define BMPC_POLICY_TRAIN_MAX_ROWS 1024
#define BMPC_POLICY_TRAIN_PAD 16          /* BMPC_POLICY_PAD of bunmpc_policy.h */

/* one fp32 device array per parameter, as torch's state_dict holds them: W[l] [N_l][K_l] row-major, b[l] [N_l] for l = 0 .. n_layers
 * (the last is the output layer); gamma[l], beta[l] [n_hidden] per hidden layer, looked at with batch_norm only.  The same struct holds
 * the parameters, their gradients, and Adam's first and second moments. */
typedef struct {
    void *W[9], *b[9];
    void *gamma[8], *beta[8];
} bmpc_policy_params_t;
int bmpc_policy_params_struct_size(void);

typedef struct {
    int n_in, n_hidden, n_layers, n_out;   /* 1..512, 1..512, 1..8 hidden layers, 1..64 */
    int batch_norm;
    double eps;                       /* BatchNorm1d's eps */
    bmpc_policy_params_t p, m, v;     /* parameters, exp_avg, exp_avg_sq */
    void *running_mean[8], *running_var[8];   /* [n_hidden] fp32 device arrays, with batch_norm */
    void *work;                       /* device scratch, 16-byte aligned: activations and gradients between the kernels of one step */
    long work_bytes;                  /* bmpc_policy_train_work_bytes(...) of the rows of the largest step at least */
} bmpc_policy_train_t;
int bmpc_policy_train_struct_size(void);

/* bytes of scratch one step of n rows needs; -1 where a size is out of range */
long bmpc_policy_train_work_bytes(int n_in, int n_hidden, int n_layers, int n_out, int batch_norm, long n);

/* rows that one workgroup of the row-parallel kernels takes per pass: the sizes n at which their paths change are multiples of this */
int bmpc_policy_train_tile(void);

typedef struct {
    long n;                           /* rows, 1 <= n <= 1024; with batch_norm 2 <= n */
    const double *x;                  /* [n] rows of n_in, fp64 device */
    long x_stride;                    /* >= n_in */
    const double *y;                  /* [n] rows of n_out, fp64 device */
    long y_stride;                    /* >= n_out */
    double lr, bc1, bc2;              /* Adam's learning rate and the two bias corrections of this call's count (step g) */
    double *loss;                     /* one fp64 device scalar (step e) */
    const bmpc_policy_params_t *grads;   /* NULL, or where this step's gradients are written (host struct of device arrays) */
} bmpc_policy_step_t;
int bmpc_policy_step_struct_size(void);

/* One training step: steps a to g as 3 n_layers + 4 kernel launches on hip_stream (NULL: the default stream), asynchronous, no host
 * synchronisation, no cooperative launch, no atomics.  Kernel boundaries are the only grid-wide synchronisation. */
int bmpc_policy_train_step_device(const bmpc_policy_train_t *net, const bmpc_policy_step_t *step, void *hip_stream);

/* The packed image of bmpc_policy_pack_host (bunmpc_policy.h) written on the device from net->p and the running statistics, every bit
 * the same: s = gamma / sqrt(running_var + eps) and t = beta - running_mean * s in fp64, each rounded once.  packed: device memory of
 * packed_bytes = bmpc_policy_packed_bytes(...) bytes, 16-byte aligned.  One launch; net->work is not looked at. */
int bmpc_policy_pack_device(const bmpc_policy_train_t *net, void *packed, long packed_bytes, void *hip_stream);

/* Every call refuses with BMPC_BAD_ARG and a message naming the field, before anything is launched or written: a NULL descriptor, n_in,
 * n_hidden outside [1, 512], n_layers outside [1, 8], n_out outside [1, 64], a NULL array of p, m, v or (batch_norm) of the running
 * statistics, with batch_norm an eps that is negative or not finite, a NULL or misaligned work or work_bytes below the step's need, n
 * outside [1, 1024], n = 1 with batch_norm, NULL x, y or loss, a stride below its width, an lr that is not finite (its sign and size are
 * the caller's), a non-finite or non-positive bc1 or bc2, a NULL array of grads, a NULL or misaligned packed image or
 * packed_bytes other than the image's size. */

#ifdef __cplusplus
}
#endif
#endif
