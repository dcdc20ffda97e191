"""The CPU twin of the fp32 centroidal kernels (biconvex_admm_kernel_f32<LPP, E>, precision = 1) and the shared pieces of their tests:
a numpy restatement of the harness-form solve with the kernel's precision contract, the cases the CPU and the GPU tests run, the
ensembles a GPU result is judged by and the mutated twins that show the judgement has teeth.

The twin is written from the kernel source, one knot per "lane" (axis 1 of every array) and one independent problem per row (axis 0:
the problems of a case times the members of their ensembles, all in one call), not from oracle/oracle_np.py cast to float32.  Where each
rule comes from (biconvex_admm_body.h unless another file is named; R is the kernel's arithmetic type, float for these kernels):

  memory      every array in memory is fp64; a value becomes R at its load and fp64 again at its store: `ldz<R>` and the `(R)at(...)`
              loads of the prologue (biconvex_lanes.h: "HBM holds fp64 whatever the arithmetic type R"), the `(double)Xg[l]` stores of
              the epilogue.  X, F, P between phases rest in LDS as R (`R *zeros = reinterpret_cast<R *>(lds_raw)`).
  constants   `const R m = (R)a.c.m, rho = ..., mu = ..., beta = ...`; `const double tol = a.c.tol, exit_tol = a.c.exit_tol` ("exit tests
              are evaluated in fp64 whatever R is"); gravity `R(kGravity)`.
  L           `R L_x, L_f`: the step constants are R -- loaded `(R)(fresh_L ? L0x : *at(a.L_x ...))`, multiplied `L_f *= beta` in R,
              stored `(double)L_f`; `invL = R(2) * (R(1) / L_f)`.  The COMPARISONS take them as `(double)L_f * 0.5`.  (40, 506.25 and
              2.25e6 times powers of 1.5 are exact in fp32 for the first fifteen retries, so the fp64 oracle's constants are the same
              numbers.)  cold_start = 1 takes BMPC_L0_X / BMPC_L0_F, 0 and 2 the arrays' values (`fresh_L`).
  force step  bPk, `an = c (dt / m)`, `sp = c (X - r) dt`, applyA (`s0 += an[n] * vx` ..., feet in order, `+ bpk` last), the half
              gradient `gx = fmaR(wf, y, rho * zx)`, the step `fmaR(-gx, invL, y)`, the "SoC" projection (`s = fmaR(fx, fx, fy * fy)`,
              `zero`, `cone`, `k = fast_div(fmaR(mu2, s, mu * fz), (mu2 + R(1)) * s)`, `fmaR(mu, s, fz) * imu`; fast_div of floats
              is `a / b`, biconvex_lanes.h): all R.
  retry test  `d'Qd + rho |A d|^2 > (L/2)|d|^2` (the header's "acceptance test").  Per lane, in R: `g2 = fmaR(d, d, g2)`,
              `cv = fmaR(wf[j] * d, d, cv)` over the 3E components in order; in the force step, the `sizeof(R)` branch: A applied
              to d itself (`s0 += an[n] * vx` ... on `dv`), `e2 = s0 * s0 + ... + s5 * s5`; `cv = fmaR(rho, e2, cv)`.  The motion step
              has no such branch: there `e = rn - ry`, `e2 = fmaR(e, e, e2)`.
  decisions   `double g2s = (double)g2, cvs = (double)cv; sum2(g2s, cvs)`: the per-lane partial sums become fp64 and the segment sums
              (biconvex_lanes.h: seg_sum2) are fp64 additions; `rhs = (double)L * 0.5 * g2s`, `bt = cvs > rhs`, `done = g2s < tol * tol`,
              the reference's sqrt form inside the 1e-14 band.  BAND (the fp32 segment sums) is `sizeof(R) == sizeof(double)` only and
              CAN_CERT is false for R = float: every step of these kernels is tested, on fp64 sums.
  momentum    `cm = (R)cmtab[i]`, the table of (t_k - 1) / t_{k+1} with t_{k+1} = 1 + sqrt(1 + 4 t_k^2) / 2 (biconvex_launch.hip:
              momentum_table_kernel, fp64); `y = fmaR(cm, xn - xo, xn)` and the image `ry = fmaR(cm, rn - ro, rn)` by linearity.
              A finishing problem's x_k is latched (`last`), its counters stop (`it_f += lanes(act)`).
  motion step make_bf (`sx += cc * fx * dt`, `b3 += -cc * fx * dt / m`, `b6 += (cc fy r2 - cc fz r1) * dt`, gravity on b5), the harness
              form's cost `qd = w`, `q = -(xr * w)` with w / xr converted from the running or the terminal arrays, the CoM box
              `lb = mx + blo`, `ub = mn + bhi` of knots with a foot on the ground, the x_init rows as a diagonal term on knot 0
              (`qd += rho`, `q = fmaR(rho, pi - xi, q)`, xi = (R)x_init), applyA with the next knot's values, the half gradient
              `g = fmaR(qd, y, fmaR(rho, z, q))`, the step and `clamp_box` on the first three components.
  violation   `double v2`: "accumulated in fp64 whatever R is" -- `v2 += (double)d * (double)d + (double)di * (double)di` of the R
              differences d = w - bf and di = X_0 - xi; `P += d` in R; the segment sum and `nrm = sqrt(v2)` in fp64; `hist`, the
              ADMM exit `nrm < exit_tol` and status 2 on NaN from that number.

What the twin does NOT pin is where hipcc contracts a product into a following sum in the expressions written without fmaR (its
default for device code) and how it associates them: the two members of `order` bracket that -- 0 rounds every product, 1 fuses them and
sums the gradient's three terms in another association.  A kernel result is therefore judged against an ENSEMBLE per problem (members),
never held to one member's bits; the discrete path (every retry and exit decision) must be the same for all of them."""
import functools

import numpy as np

from bunmpc_amd import problems
from bunmpc_amd._lib import L0_F, L0_X
from tests.util import ENSEMBLE_SEED, K_SPREAD, TOL_FP64, rel_l2

GRAVITY = 9.81
ULP32 = 2.0 ** -23          # one fp32 ulp: the least any fp32 result can promise
MARGIN = 1e-4               # every decision of every member is at least this far from its threshold, relative
N_PERTURBED = 4
L_F_RETRY = 40.0            # regimes b and c start the force step here: every case backtracks
MUTANTS = ("weight", "imagediff", "droplane")

# (lanes per problem, H, B, config): B ragged against the problems per wave of the mapping
CASES = [(16, 3, 6, "solo12_trot"), (16, 3, 6, "biped_walk"), (16, 15, 6, "solo12_trot"), (16, 15, 6, "biped_walk"),
         (32, 20, 5, "solo12_trot"), (32, 20, 5, "biped_walk"), (32, 20, 5, "solo12_mixed"),
         (32, 31, 5, "solo12_trot"), (32, 31, 5, "biped_walk"), (32, 31, 5, "solo12_mixed"),
         (64, 40, 3, "go2_bound"), (64, 63, 3, "solo12_trot"), (64, 63, 3, "biped_walk")]
REGIMES = ("a", "b", "c")
# Regime r, the reference's own tolerances (tol = 1e-5, maxit = 150, ten ADMM iterations, cold): steps shrink to a few fp32 ulp of the
# forces, the exits of fp32 runs no longer agree, so trace is NOT pinned there -- the retry decisions are: the counts of
# retries and the step constants a solve returns.  That is where the `sizeof(R)` branch of the force step's retry test (A applied to d,
# not the difference of the images) decides: with the difference the test fires on the images' rounding and L_f runs to +inf.
R_CASES = [(16, 3, 6, "biped_walk"), (16, 15, 6, "solo12_trot"), (16, 15, 6, "biped_walk"), (32, 20, 5, "biped_walk"), (32, 20, 5, "solo12_mixed"),
           (64, 63, 3, "biped_walk")]
# The seed of a case's random warm start (regime b) where seed 0 left a problem unfit (tests/test_f32_cpu.py: test_twin_is_fit_to_judge).
# What goes wrong is the algorithm's, in fp64 as in fp32: from forces of N(3, 4^2) and L_f = 40 the reference's "SoC" step (squared
# norm against mu fz: not a projection, it can expand) lets the forces of a mu = 1 robot grow until the motion step's retry test is
# decided by the rounding of its images -- tens to hundreds of motion retries whose count differs between fp32 and fp64.  The first
# seed at which no problem of the case does that: 2, 1 and (three problems of 63 knots) 28.
SEEDS = {"32-31-solo12_mixed": 2, "64-40-go2_bound": 1, "64-63-solo12_trot": 28}
# per case and regime: what had to move for the margin condition (MARGIN) to hold on every problem -- {(lanes, H, config, regime): dict(tol=...)}
OVERRIDES = {}


def case_id(c):
    return "%d-%d-%s" % (c[0], c[1], c[3])


def momentum_table(n):
    """(t_k - 1) / t_{k+1}, fp64 (biconvex_launch.hip: momentum_table_kernel)"""
    tab, tk = np.empty(n), 1.0
    for i in range(n):
        tk1 = 1.0 + np.sqrt(1.0 + 4.0 * tk * tk) * 0.5
        tab[i] = (tk - 1.0) / tk1
        tk = tk1
    return tab


class _Arith:
    """the arithmetic type R and the two ways an unfused source expression may have been compiled"""

    def __init__(self, dtype, order):
        self.R, self.order, self.wide = dtype, order, dtype == np.float64

    def c(self, x):
        """a value of memory (fp64) converted to R"""
        return np.asarray(x, dtype=np.float64).astype(self.R)

    def fma(self, a, b, c):
        """fmaR: the product of two floats is exact in fp64; the sum is rounded there and then to float"""
        if self.wide:
            return a * b + c
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)

    def mad(self, a, b, c):
        """a * b + c as written without fmaR: rounded product (order 0) or contracted (order 1)"""
        return self.fma(a, b, c) if self.order else a * b + c


def _next(v):
    """the value of knot t + 1 (0 behind the last lane: every use of that lane's value is masked in the kernel)"""
    o = np.zeros_like(v)
    o[:, :-1] = v[:, 1:]
    return o


def _prev(v):
    o = np.zeros_like(v)
    o[:, 1:] = v[:, :-1]
    return o


def _row(a, rows):
    return np.broadcast_to(a[0], (len(rows),) + a.shape[1:]) if a.shape[0] == 1 else a[rows]


def solve(b, rows=None, x_init=None, warm=None, L_x=None, L_f=None, cold_start=None, num_iters=2, maxit=8, tol=0.0, exit_tol=1e-3,
          beta=1.5, mu=None, dtype=np.float32, order=0, mutant=None):
    """The harness-form solve of problems `rows` of batch b (default: all; a problem may appear more than once), one per row, as the fp32
    kernel computes it (dtype=np.float64: the same algebra in fp64).  x_init (len(rows), 9) replaces the batch's; warm = (X, F, P) per row or
    None for a cold start; L_x / L_f: the step constants in the arrays, taken unless cold_start == 1 (default: 1 without warm, else 0; 2
    = cold iterates, the arrays' constants).  mutant: one of MUTANTS.  Returns X, F, P, L_x, L_f (fp64, as stored), hist, trace, stats,
    dyn_viol like batch.solve_host(keep_hist=True), and `margin` (rows, 5): the smallest relative distance of a decision from its
    threshold -- force retry, force exit, motion retry, motion exit, ADMM exit (inf where the threshold is 0 or no decision was taken)."""
    ar = _Arith(dtype, order)
    R, fma, mad = ar.R, ar.fma, ar.mad
    rows = np.arange(b.B) if rows is None else np.asarray(rows)
    M, H, E = len(rows), b.H, b.E
    K, NF = H + 1, 3 * E
    cold_start = (1 if warm is None else 0) if cold_start is None else cold_start
    rv = (np.arange(K) < H)[None, :]                         # lanes that own a dynamics row block and a force block
    one, two, half = R(1), R(2), R(0.5)
    m, rho, beta_r, g = R(b.m), R(b.rho), R(beta), R(GRAVITY)
    mu = R(b.mu if mu is None else mu)
    tol2 = tol * tol
    cmtab = momentum_table(maxit)

    def lanes(a, width):                                     # a per-knot input array (M, H * width) -> (M, K, width), zero in the last lane
        o = np.zeros((M, K, width), dtype=R)
        o[:, :H] = ar.c(a).reshape(M, H, width)
        return o
    dt = lanes(b.dt[rows], 1)[..., 0]
    dtp = _prev(dt)
    cnt = lanes(b.cnt_plan[rows], 4 * E).reshape(M, K, E, 4)
    cn, rr = cnt[..., 0], cnt[..., 1:4]
    wf = lanes(_row(b.W_F, rows), NF).reshape(M, K, E, 3).copy()
    if mutant == "weight":                                   # one force weight of one knot: z of the knot's first foot on the ground
        kk = H // 2
        for i in range(M):
            on = np.nonzero(cn[i, kk] > 0)[0]
            wf[i, kk, on[0] if on.size else 0, 2] *= R(1.0 + 1e-4)
    xi = ar.c(b.x_init[rows] if x_init is None else x_init)
    # the motion cost and bounds (create_cost_X, create_bound_constraints), per lane
    w = np.concatenate([ar.c(_row(b.W_X, rows)).reshape(M, H, 9), ar.c(_row(b.W_X_ter, rows)).reshape(M, 1, 9)], axis=1)
    xr = np.concatenate([ar.c(b.X_nom[rows]).reshape(M, H, 9), ar.c(b.X_ter[rows]).reshape(M, 1, 9)], axis=1)
    qd0, q0 = w, -(xr * w)
    bnd = lanes(_row(b.bounds, rows).reshape(M, -1), 6)
    bounded = rv & (cn.sum(axis=2, dtype=R) > 0)             # (csum += c[n]: contact flags, exact)
    lb = np.where(bounded[..., None], rr.max(axis=2) + bnd[..., 0:3], R(-np.inf))
    ub = np.where(bounded[..., None], rr.min(axis=2) + bnd[..., 3:6], R(np.inf))
    l0 = (np.arange(K) == 0)[None, :, None]

    # iterates on chip
    if cold_start != 0:
        Xg = np.repeat(xi[:, None, :], K, axis=1)
        Fg, Pg, PI = np.zeros((M, K, E, 3), R), np.zeros((M, K, 9), R), np.zeros((M, 9), R)
    else:
        X0, F0, P0 = (np.asarray(a, dtype=np.float64).reshape(M, -1) for a in warm)
        Xg = ar.c(X0).reshape(M, K, 9).copy()
        Fg = lanes(F0, NF).reshape(M, K, E, 3).copy()
        Pg = lanes(P0[:, :9 * H], 9).copy()
        PI = ar.c(P0[:, 9 * H:]).copy()
    Lx = ar.c(np.broadcast_to(L0_X if (cold_start == 1 or L_x is None) else L_x, (M,))).copy()
    Lf = ar.c(np.broadcast_to(L0_F if (cold_start == 1 or L_f is None) else L_f, (M,))).copy()
    n_admm, it_f, it_x, bt_f, bt_x, status = (np.zeros(M, np.int64) for _ in range(6))
    last_viol = np.zeros(M)
    hist = np.full((M, max(num_iters, 1)), np.nan)
    trace = np.full((M, max(num_iters, 1), 4), -1, np.int64)
    margin = np.full((M, 5), np.inf)
    alive = np.ones(M, bool)

    def note(col, who, value, threshold):
        """the relative distance of a decision's two sides, for the rows that took it"""
        with np.errstate(divide="ignore", invalid="ignore"):
            dist = np.where(threshold != 0, np.abs(value / threshold - 1.0), np.inf)
        dist = np.where(np.isnan(dist), 0.0, dist)
        margin[who, col] = np.minimum(margin[who, col], dist[who])

    def decide(g2, cv, L, pend, act, cols):
        """retry and exit of a step from the per-lane partial sums (R): fp64 segment sums, fp64 comparisons"""
        g2s, cvs = g2.astype(np.float64).sum(axis=1), cv.astype(np.float64).sum(axis=1)
        Lh = L.astype(np.float64) * 0.5
        with np.errstate(invalid="ignore", over="ignore"):
            rhs = Lh * g2s
            bt, done = cvs > rhs, g2s < tol2
            edge = (np.abs(cvs - rhs) <= 1e-14 * rhs) | (np.abs(g2s - tol2) <= 1e-14 * tol2)
            Gn = np.sqrt(g2s)
            bt = np.where(edge, cvs > Lh * (Gn * Gn), bt)
            done = np.where(edge, Gn < tol, done)
        note(cols[0], pend, cvs, rhs)
        note(cols[1], pend, g2s, np.full(M, tol2))
        return bt & pend, done

    def fista(step, x, image, L, counts, act, latch):
        """the FISTA loop of a phase (fista.cpp:6-47 as the kernel runs it): step(y, ry, invL) -> (xn, rn, g2, cv)"""
        its, bts, cols = counts
        y, ry, xo, ro = x, image, x, image
        for i in range(maxit):
            if not act.any():
                break
            cm = R(cmtab[i])
            pend = act.copy()
            while True:
                invL = two * (one / L)
                xn, rn, g2, cv = step(y, ry, invL)
                bt, done = decide(g2, cv, L, pend, act, cols)
                pend = bt
                if not bt.any():
                    break
                L[bt] = L[bt] * beta_r
                bts[bt] += 1
            latch(act & (done | (i == maxit - 1)), xn)
            y, ry = fma(cm, xn - xo, xn), fma(cm, rn - ro, rn)
            xo, ro = xn, rn
            its += act
            act = act & ~done

    def ex(a, n):                                            # a per-row value against arrays with n more axes
        return a.reshape(a.shape + (1,) * n)

    for it in range(num_iters):
        if not alive.any():
            break
        # ------------------------------------------------------------------ F step
        X = Xg
        bx = _next(X[..., 3:9]) - X[..., 3:9]
        bx[..., 2] = mad(g, dt, bx[..., 2])
        bpk = np.where(rv[..., None], -bx + Pg[..., 3:9], R(0))
        an = cn * (dt / m)[..., None]
        sp = cn[..., None] * (X[:, :, None, 0:3] - rr) * dt[..., None, None]

        def apply_Ax(v, add):
            s = [np.zeros((M, K), R) for _ in range(6)]
            for n in range(E):
                vx, vy, vz = v[:, :, n, 0], v[:, :, n, 1], v[:, :, n, 2]
                a_, s0, s1, s2 = an[:, :, n], sp[:, :, n, 0], sp[:, :, n, 1], sp[:, :, n, 2]
                s[0], s[1], s[2] = mad(a_, vx, s[0]), mad(a_, vy, s[1]), mad(a_, vz, s[2])
                if ar.order:
                    s[3] = s[3] + fma(s2, vy, -(s1 * vz)); s[4] = s[4] + fma(s0, vz, -(s2 * vx)); s[5] = s[5] + fma(s1, vx, -(s0 * vy))
                else:
                    s[3] = s[3] + (s2 * vy - s1 * vz); s[4] = s[4] + (s0 * vz - s2 * vx); s[5] = s[5] + (s1 * vx - s0 * vy)
            u = np.stack(s, axis=-1)
            return u + bpk if add else u

        def force_step(y, ry, invL):
            r0, r1, r2, r3, r4, r5 = (ry[..., k, None] for k in range(6))
            a_, s0, s1, s2 = an, sp[..., 0], sp[..., 1], sp[..., 2]
            if ar.order:
                zx = fma(a_, r0, fma(s1, r5, -(s2 * r4))); zy = fma(a_, r1, fma(s2, r3, -(s0 * r5))); zz = fma(a_, r2, fma(s0, r4, -(s1 * r3)))
            else:
                zx = a_ * r0 - s2 * r4 + s1 * r5; zy = a_ * r1 + s2 * r3 - s0 * r5; zz = a_ * r2 - s1 * r3 + s0 * r4
            gr = fma(wf, y, rho * np.stack([zx, zy, zz], axis=-1))
            fr = fma(-gr, ex(invL, 3), y)
            s = fma(fr[..., 0], fr[..., 0], fr[..., 1] * fr[..., 1])
            fz = fr[..., 2]
            zero = (s * mu < -fz) | (fz < 0)
            cone = ~zero & (s > mu * fz)
            mu2 = mu * mu
            imu = one / (mu * mu + one)
            with np.errstate(divide="ignore", invalid="ignore"):
                k = fma(mu2, s, mu * fz) / ((mu2 + one) * s)
                keep = np.where(zero, R(0), one)
                xn = np.stack([np.where(cone, fr[..., 0] * k, keep * fr[..., 0]), np.where(cone, fr[..., 1] * k, keep * fr[..., 1]),
                               np.where(cone, fma(mu, s, fz) * imu, keep * fz)], axis=-1)
            rn = apply_Ax(xn, True)
            dv = xn - y
            g2, cv = np.zeros((M, K), R), np.zeros((M, K), R)
            for n in range(E):
                for k in range(3):
                    d = dv[:, :, n, k]
                    g2 = fma(d, d, g2)
                    cv = fma(wf[:, :, n, k] * d, d, cv)
            if mutant == "imagediff":
                e, e2 = rn - ry, np.zeros((M, K), R)
                for k in range(6):
                    e2 = fma(e[..., k], e[..., k], e2)
            else:
                s = apply_Ax(dv, False)
                e2 = s[..., 0] * s[..., 0]
                for k in range(1, 6):
                    e2 = mad(s[..., k], s[..., k], e2)
            cv = fma(rho, e2, cv)
            if mutant == "droplane":
                g2 = g2.copy()
                g2[:, H - 1] = 0
            return xn, rn, g2, cv

        def latch_f(who, xn):
            Fg[who] = xn[who]
        x0 = Fg.copy()
        fista(force_step, x0, apply_Ax(x0, True), Lf, (it_f, bt_f, (0, 1)), alive.copy(), latch_f)

        # ------------------------------------------------------------------ X step
        cf = cn[..., None] * Fg                                                       # cc[n] * f
        SX, SY, SZ = (np.zeros((M, K), R) for _ in range(3))
        bf = [np.zeros((M, K), R) for _ in range(9)]
        for n in range(E):
            cx, cy, cz = cf[:, :, n, 0], cf[:, :, n, 1], cf[:, :, n, 2]
            SX, SY, SZ = mad(cx, dt, SX), mad(cy, dt, SY), mad(cz, dt, SZ)
            bf[3] = bf[3] + -cx * dt / m; bf[4] = bf[4] + -cy * dt / m; bf[5] = bf[5] + -cz * dt / m
            r0, r1, r2 = rr[:, :, n, 0], rr[:, :, n, 1], rr[:, :, n, 2]
            if ar.order:
                bf[6] = mad(fma(cy, r2, -(cz * r1)), dt, bf[6]); bf[7] = mad(fma(cz, r0, -(cx * r2)), dt, bf[7]); bf[8] = mad(fma(cx, r1, -(cy * r0)), dt, bf[8])
            else:
                bf[6] = bf[6] + (cy * r2 - cz * r1) * dt; bf[7] = bf[7] + (cz * r0 - cx * r2) * dt; bf[8] = bf[8] + (cx * r1 - cy * r0) * dt
        bf[5] = mad(g, dt, bf[5])
        bf = np.stack(bf, axis=-1)
        bpk9 = np.where(rv[..., None], -bf + Pg, R(0))
        bpi = np.where(l0, (PI - xi)[:, None, :], R(0))
        qd = qd0 + np.where(l0, rho, R(0))
        q = fma(rho, bpi, q0)
        sx, sy, sz, dte, dtpe = SX[..., None], SY[..., None], SZ[..., None], dt[..., None], dtp[..., None]

        def apply_Af(v, add):
            vn = _next(v)
            wv = v - vn
            wv[..., 0:3] = mad(dte, vn[..., 3:6], wv[..., 0:3])
            if ar.order:
                wv[..., 6] += fma(SY, v[..., 2], -(SZ * v[..., 1])); wv[..., 7] += fma(SZ, v[..., 0], -(SX * v[..., 2])); wv[..., 8] += fma(SX, v[..., 1], -(SY * v[..., 0]))
            else:
                wv[..., 6] += SY * v[..., 2] - SZ * v[..., 1]; wv[..., 7] += SZ * v[..., 0] - SX * v[..., 2]; wv[..., 8] += SX * v[..., 1] - SY * v[..., 0]
            return np.where(rv[..., None], wv + bpk9 if add else wv, R(0))

        def motion_step(y, ry, invL):
            wp = _prev(ry)
            z = ry - wp
            z[..., 3:6] = fma(dtpe, wp[..., 0:3], z[..., 3:6])
            if ar.order:
                z[..., 0] += fma(SZ, ry[..., 7], -(SY * ry[..., 8])); z[..., 1] += fma(SX, ry[..., 8], -(SZ * ry[..., 6])); z[..., 2] += fma(SY, ry[..., 6], -(SX * ry[..., 7]))
            else:
                z[..., 0] += SZ * ry[..., 7] - SY * ry[..., 8]; z[..., 1] += SX * ry[..., 8] - SZ * ry[..., 6]; z[..., 2] += SY * ry[..., 6] - SX * ry[..., 7]
            gr = fma(qd, y, fma(rho, z, q))
            xn = fma(-gr, ex(invL, 2), y)
            xn[..., 0:3] = np.maximum(np.minimum(xn[..., 0:3], ub), lb)
            rn = apply_Af(xn, True)
            d, e = xn - y, rn - ry
            g2, cv, e2 = (np.zeros((M, K), R) for _ in range(3))
            for l in range(9):
                g2 = fma(d[..., l], d[..., l], g2)
                cv = fma(qd[..., l] * d[..., l], d[..., l], cv)
                e2 = fma(e[..., l], e[..., l], e2)
            cv = fma(rho, e2, cv)
            if mutant == "droplane":
                g2 = g2.copy()
                g2[:, H] = 0
            return xn, rn, g2, cv

        def latch_x(who, xn):
            Xg[who] = xn[who]
        x0 = Xg.copy()
        fista(motion_step, x0, apply_Af(x0, True), Lx, (it_x, bt_x, (2, 3)), alive.copy(), latch_x)

        # ------------------------------------------------------------------ dyn_violation = A_f X - b_f; P += dyn_violation
        fin = Xg
        d = np.where(rv[..., None], apply_Af(fin, False) - bf, R(0))
        di = np.where(l0, fin - xi[:, None, :], R(0))
        v2 = np.zeros((M, K))
        for l in range(9):
            v2 = v2 + (d[..., l].astype(np.float64) * d[..., l].astype(np.float64) + di[..., l].astype(np.float64) * di[..., l].astype(np.float64))
        Pg[alive] = (Pg + d)[alive]
        PI[alive] = (PI + di[:, 0, :])[alive]
        with np.errstate(invalid="ignore"):
            nrm = np.sqrt(v2.sum(axis=1))
        last_viol[alive] = nrm[alive]
        hist[alive, it] = nrm[alive]
        n_admm += alive
        trace[alive, it] = np.stack([it_f, it_x, bt_f, bt_x], axis=1)[alive]
        status[alive & np.isnan(nrm)] = 2
        note(4, alive, nrm, np.full(M, exit_tol))
        with np.errstate(invalid="ignore"):
            alive = alive & ~(np.isnan(nrm) | (nrm < exit_tol))

    assert all(a.dtype == R for a in (Xg, Fg, Pg, PI, Lx, Lf)), "an operation of the twin left the arithmetic type"
    P = np.concatenate([Pg[:, :H].reshape(M, -1), PI], axis=1).astype(np.float64)
    return dict(X=Xg.reshape(M, -1).astype(np.float64), F=Fg[:, :H].reshape(M, -1).astype(np.float64), P=P, L_x=Lx.astype(np.float64),
                L_f=Lf.astype(np.float64), hist=hist, trace=trace, dyn_viol=last_viol,
                stats=np.stack([n_admm, it_f, it_x, bt_f, bt_x, status], axis=1), margin=margin)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch(case):
    """(the case's batch, its random forces (B, 3EH) for the warm start of regime b: N((0, 0, 3), 4^2) per foot, as tests/cone_np.py draws
    them), fixed per case"""
    lanes, H, B, config = case
    b = problems.make_batch(config, B, H=H)
    rng = np.random.default_rng([20251018, H, b.E, B, SEEDS.get(case_id(case), 0)])
    F = rng.normal(0.0, 4.0, size=(B, H, b.E, 3)) + np.array([0.0, 0.0, 3.0])
    return b, F.reshape(B, -1)


def settings(case, regime):
    """the solve of a case in a regime: dict(num_iters, maxit, tol, exit_tol, warm, L_x, L_f) -- the keyword arguments batch.solve_host,
    oracle_c.solve_batch and solve() share (L_x, L_f: one value per problem) -- and cold_start
      a  fixed length: tol = 0, maxit = 8, two ADMM iterations (one at H = 63), cold, exit_tol = 0 (no ADMM early exit)
      b  retries: a with a warm start (random F, P = 0) and L_f = 40
      c  exits: tol = 1e-3, maxit = 150, L_f = 40 from the cold start's iterates: the FISTA exit and the retry test both decide
      k  carried step constants: a with cold_start = 2, which keeps the arrays' L_f = 40 (batch.DeviceBatch only)
      r  the reference's tolerances (R_CASES only): retry counts and step constants pinned, trace not"""
    b, F = batch(case)
    X, F0, P = b.warm_start()
    iters = 1 if b.H == 63 else 2
    s = dict(a=dict(num_iters=iters, maxit=8, tol=0.0, exit_tol=0.0, warm=None, L_f=L0_F),
             b=dict(num_iters=iters, maxit=8, tol=0.0, exit_tol=0.0, warm=(X, F, P), L_f=L_F_RETRY),
             c=dict(num_iters=iters, maxit=150, tol=1e-3, exit_tol=0.0, warm=(X, F0, P), L_f=L_F_RETRY),
             k=dict(num_iters=iters, maxit=8, tol=0.0, exit_tol=0.0, warm=None, L_f=L_F_RETRY),
             r=dict(num_iters=10, maxit=150, tol=1e-5, exit_tol=0.0, warm=None, L_f=L0_F))[regime]
    s["cold_start"] = {"a": 1, "r": 1, "k": 2}.get(regime, 0)
    s["L_f"] = np.broadcast_to(np.asarray(s["L_f"], dtype=np.float64), (b.B,)).copy()
    s["L_x"] = np.broadcast_to(np.asarray(s.get("L_x", L0_X), dtype=np.float64), (b.B,)).copy()
    s.update(OVERRIDES.get((case[0], case[1], case[3], regime), {}))
    return s


def perturbed_x_init(b, member):
    """x_init of every problem moved by one fp32 ulp per component on the float32 grid, direction drawn as tests/util.py:
    ulp_perturbed_x_init draws it -- from (ENSEMBLE_SEED, problem index, member)"""
    xi = np.array(b.x_init, dtype=np.float64).astype(np.float32)
    for i in range(b.B):
        up = np.random.default_rng([ENSEMBLE_SEED, i, int(member)]).integers(0, 2, size=xi.shape[1]) > 0
        xi[i] = np.nextafter(xi[i], np.where(up, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    return xi.astype(np.float64)


def run(case, regime, order=0, perturbed=None, dtype=np.float32, mutant=None):
    """the twin on every problem of the case: one member of the ensemble (perturbed: None or the member number of the x_init move)"""
    b = batch(case)[0]
    s = settings(case, regime)
    return solve(b, x_init=None if perturbed is None else perturbed_x_init(b, perturbed), warm=s["warm"], L_x=s["L_x"], L_f=s["L_f"], num_iters=s["num_iters"],
                 maxit=s["maxit"], tol=s["tol"], exit_tol=s["exit_tol"], cold_start=s["cold_start"], dtype=dtype, order=order, mutant=mutant)


@functools.lru_cache(maxsize=None)
def members(case, regime):
    """the ensemble of a case: the twin in both orders, each also with x_init moved in N_PERTURBED seeded directions -- ten results, each of
    every problem of the case, computed in two calls (the moved x_init are further rows) and once per process: do not modify them"""
    b = batch(case)[0]
    s = settings(case, regime)
    B = b.B
    rows = np.tile(np.arange(B), 1 + N_PERTURBED)
    xi = np.concatenate([b.x_init] + [perturbed_x_init(b, k) for k in range(N_PERTURBED)])
    warm = None if s["warm"] is None else tuple(np.tile(a, (1 + N_PERTURBED, 1)) for a in s["warm"])
    out = []
    for order in (0, 1):
        r = solve(b, rows=rows, x_init=xi, warm=warm, L_x=np.tile(s["L_x"], 1 + N_PERTURBED), L_f=np.tile(s["L_f"], 1 + N_PERTURBED), num_iters=s["num_iters"], maxit=s["maxit"], tol=s["tol"],
                  exit_tol=s["exit_tol"], cold_start=s["cold_start"], order=order)
        out += [{k: v[j * B:(j + 1) * B] for k, v in r.items()} for j in range(1 + N_PERTURBED)]
    return out


def oracle_solve(oracle, case, regime):
    """the strict fp64 C oracle on the case (oracle: oracle.oracle_c), with hist and trace"""
    b = batch(case)[0]
    s = settings(case, regime)
    return oracle.solve_batch(b, num_iters=s["num_iters"], maxit=s["maxit"], tol=s["tol"], exit_tol=s["exit_tol"], warm=s["warm"], L_x=s["L_x"], L_f=s["L_f"], trace=True)


def distance(got, ref):
    """per problem: max(rel-L2 X, F, P) of a result from the reference, and the largest relative distance of hist over the ADMM iterations"""
    e = np.maximum.reduce([rel_l2(got[k], ref[k]) for k in "XFP"])
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.abs(got["hist"] - ref["hist"]) / np.abs(ref["hist"])
    return e, np.where(np.isnan(h), np.where(np.isnan(got["hist"]) == np.isnan(ref["hist"]), 0.0, np.inf), h).max(axis=1)


def ensemble_bounds(ens, ref, floor=ULP32):
    """per problem: y (values) and y_hist, the largest distance of any member of the ensemble from the oracle, and the bounds
    K_SPREAD * max(y, floor) a kernel result is held to (floor: one fp32 ulp)"""
    d = [distance(r, ref) for r in ens]
    y, yh = np.max([a for a, _ in d], axis=0), np.max([h for _, h in d], axis=0)
    return dict(y=y, y_hist=yh, bound=K_SPREAD * np.maximum(y, floor), bound_hist=K_SPREAD * np.maximum(yh, floor))


def judge(got, ens, ref, exact=True):
    """A result (the kernel's, a mutant's) against the case's ensemble and oracle: dict(path: per problem, trace / stats / L_x / L_f equal
    the oracle's -- exact=False (regime r): the retry counts, the ADMM count, the status and L_x / L_f; err, err_hist, ratio = err / y,
    ratio_hist; ok: per problem, everything within its bound).  exact=False takes the floor of the value bounds from tests/util.py: TOL_FP64
    = 1e-5, the agreement the project asks of two solves at the reference's tolerances -- fp32 rounding of the iterates (6e-8 x 10 N x
    sqrt(240) ~ 1e-5) is the size of the absolute exit threshold there, so runs that exit an iteration apart differ by
    that much whatever their ensemble says."""
    bnd = ensemble_bounds(ens, ref, ULP32 if exact else TOL_FP64)
    cols = slice(None) if exact else [0, 3, 4, 5]
    path = np.array([(not exact or np.array_equal(got["trace"][i], ref["trace"][i])) and np.array_equal(got["stats"][i, cols], ref["stats"][i, cols])
                     and got["L_x"][i] == ref["L_x"][i] and got["L_f"][i] == ref["L_f"][i] for i in range(len(bnd["y"]))])
    e, h = distance(got, ref)
    return dict(path=path, err=e, err_hist=h, ratio=e / np.maximum(bnd["y"], ULP32), ratio_hist=h / np.maximum(bnd["y_hist"], ULP32),
                ok=path & (e <= bnd["bound"]) & (h <= bnd["bound_hist"]), **bnd)
