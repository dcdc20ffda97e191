"""Plain-numpy references and inputs for the per-pass checks of the IK-DDP kernels (tests/test_ik_passes_cpu.py runs them against
the CPU twins, tests/test_ik_passes_gpu.py against ik_calcdiff_kernel / ik_calcdiff1_kernel / ik_backward_kernel<1|2> through
bmpc_ik_selftest_passes):
  * unpack_node: the compact per-node hand-over of the derivative pass (ik_types.h: kLqqDoubles / kHnDoubles, written by
    calc_assemble in ik_ddp.hip) back into the dense L_xx, F_x, F_u of crocoddyl's ActionData;
  * riccati: the backward pass of oracle/ik_ddp_np.py::solve_ddp on its own, generic in the number type (np.float64 or
    np.longdouble: no LAPACK, no BLAS), with SolverDDP's regularisation retries;
  * the fixed-seed case set, the two CPU twins evaluated on it, the error measures and the tolerances both test files use.
TEST INFRASTRUCTURE ONLY."""
import contextlib
import os

import numpy as np

from bunmpc_amd import urdf_model
from oracle import ik_ddp_np, ik_oracle_c as ic, rbd_np as rb

NX, NDX, NV, NQ, NTASK = 37, 36, 18, 19, 33
LQQ, HN, HN_W, HN_D11, HN_D22 = 296, 248, 216, 224, 240         # ik_types.h
SCAL = dict(cost=0, xreg=1, d1=2, d2=3, stop=4, feas=5, wasfeas=6, done=7, iters=8, recalc=9, status=10)
LAYOUT_KEYS = ("xs", "us", "scal", "K", "kff", "fs", "Lx", "Lqq", "xnext", "Hn", "Lu", "Luu", "A6", "B6", "nrs", "njl", "ncs", "total",
               "node_cost")
ROBOTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bunmpc_amd", "robots")
EPS = float(np.finfo(np.float64).eps)


def layout(T):
    """offsets (doubles) into a problem's workspace, from the library (host code, no GPU)"""
    import ctypes as C
    from bunmpc_amd import _lib
    off = (C.c_long * len(LAYOUT_KEYS))()
    n = _lib.lib().bmpc_ik_layout_all(T, off, len(LAYOUT_KEYS))
    assert n == len(LAYOUT_KEYS), n
    return dict(zip(LAYOUT_KEYS, list(off)))


# ------------------------------------------------------------------- the compact hand-over ---
def unpack_lxx(lqq, hn, mut=None):
    """dense L_xx (36 x 36) of a node from its kLqqDoubles + kHnDoubles:
         L_xx = [L_qq' 0; 0 0] + (sc wm) M^T M + diag(0_18, sc wst sw_v)
       L_qq': tile (0,0) (rows / columns 0..15) as the MFMA accumulator holds it, [v][lane] with row = (lane >> 4) + 4 v and
       column = lane & 15; columns 16, 17 of tile (0,1) as [row][2] (the mirror image is not stored); the 2 x 2 corner of tile (1,1).
       M (6 x 36) row-major, sc wm at kHnW, the velocity diagonal by column of tile (1,1) (d11[c] = state index 16 + c, c >= 2) and of
       tile (2,2) (d22[c] = state index 32 + c)."""
    L = np.zeros((NDX, NDX), dtype=lqq.dtype)
    t00 = lqq[:256].reshape(4, 4, 16)                # [v][lane >> 4][lane & 15]
    for v in range(4):
        for lk in range(4):
            L[lk + 4 * v, :16] = t00[v, lk]
    t01 = lqq[256:288].reshape(2, 16).T if mut == "tile01_transposed" else lqq[256:288].reshape(16, 2)
    L[:16, 16:18] = t01
    L[16:18, :16] = t01.T
    L[16:18, 16:18] = lqq[288:292].reshape(2, 2)
    M = hn[:216].reshape(6, NDX)
    L += hn[HN_W] * (M.T @ M)
    if mut != "no_velocity_diagonal":
        for c in range(2, 16):
            L[16 + c, 16 + c] += hn[HN_D11 + c]
        for c in range(4):
            L[32 + c, 32 + c] += hn[HN_D22 + c]
    return L


def dense_F(A6, B6, dt, dtype=np.float64):
    """F_x = [[A, dt B], [0, I]], F_u = [[dt^2 B], [dt I]] with A = blockdiag(A6, I_12), B = blockdiag(B6, I_12): the Jintegrate blocks
    of the Euler step (row-major 6 x 6, as euler_step leaves them)"""
    A, Bm = np.eye(NV, dtype=dtype), np.eye(NV, dtype=dtype)
    A[:6, :6] = np.asarray(A6).reshape(6, 6)
    Bm[:6, :6] = np.asarray(B6).reshape(6, 6)
    Fx = np.eye(NDX, dtype=dtype)
    Fx[:NV, :NV] = A
    Fx[:NV, NV:] = dt * Bm
    Fu = np.vstack([dt * dt * Bm, dt * np.eye(NV, dtype=dtype)])
    return Fx, Fu


def unpack_node(ws_row, lay, t, dt, T, mut=None):
    """node t of one problem's workspace row -> dict(Lx, Lxx[, Lu, Luu (diagonal), Fx, Fu, xnext]) as dense as the twins give them;
    dt: the node's time step (ignored at the terminal node t == T)"""
    lqq = ws_row[lay["Lqq"] + t * LQQ: lay["Lqq"] + (t + 1) * LQQ]
    hn = ws_row[lay["Hn"] + t * HN: lay["Hn"] + (t + 1) * HN]
    out = dict(Lx=ws_row[lay["Lx"] + t * NDX: lay["Lx"] + (t + 1) * NDX].copy(), Lxx=unpack_lxx(lqq, hn, mut))
    if t < T:
        out["Lu"] = ws_row[lay["Lu"] + t * NV: lay["Lu"] + (t + 1) * NV].copy()
        out["Luu"] = ws_row[lay["Luu"] + t * NV: lay["Luu"] + (t + 1) * NV].copy()
        out["xnext"] = ws_row[lay["xnext"] + t * NX: lay["xnext"] + (t + 1) * NX].copy()
        out["Fx"], out["Fu"] = dense_F(ws_row[lay["A6"] + 36 * t: lay["A6"] + 36 * (t + 1)], ws_row[lay["B6"] + 36 * t: lay["B6"] + 36 * (t + 1)], dt)
    return out


# ------------------------------------------------------------------------ the Riccati pass ---
def _mm(a, b):
    return np.einsum("ij,jk->ik", a, b)          # (einsum: numpy's own loops for every dtype, the same code path for both)


def _mv(a, x):
    return np.einsum("ij,j->i", a, x)


def cholesky_lower(A):
    """lower factor by columns, or None at a pivot that is not > 0 (Eigen::LLT info != Success)"""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - _mv(L[j + 1:, :j], L[j, :j])) / L[j, j]
    return L


def _solve_llt(L, Bm):
    """(L L^T)^-1 Bm, Bm a matrix or a vector"""
    n = L.shape[0]
    Y = np.array(Bm, dtype=L.dtype, copy=True)
    for i in range(n):
        Y[i] = (Y[i] - np.tensordot(L[i, :i], Y[:i], axes=(0, 0))) / L[i, i]
    for i in range(n - 1, -1, -1):
        Y[i] = (Y[i] - np.tensordot(L[i + 1:, i], Y[i + 1:], axes=(0, 0))) / L[i, i]
    return Y


def riccati(data, fs, xreg, feasible, dtype, mut=None, reg_max=1e9):
    """SolverDDP::backwardPass with solve()'s retries: data[t] = dict(Lx, Lxx, Lu, Luu (matrix or its diagonal), Fx, Fu) for t < T,
    dict(Lx, Lxx) for t = T; fs [T+1][36] gaps (used when not feasible).  On a non-positive pivot or a non-finite V the
    regularisation (xreg = ureg) is multiplied by 10 and the pass starts again at the terminal node; at reg_max it gives up.
    Returns dict(K [T][18][36], k [T][18], d1, d2, stop, reg, retries, gave_up)."""
    T = len(data) - 1
    c = lambda a: np.asarray(a, dtype=dtype)                   # noqa: E731
    D = []
    for t, d in enumerate(data):
        e = dict(Lx=c(d["Lx"]), Lxx=c(d["Lxx"]))
        if t < T:
            Luu = c(d["Luu"])
            e.update(Lu=c(d["Lu"]), Luu=np.diag(Luu) if Luu.ndim == 1 else Luu, Fx=c(d["Fx"]), Fu=c(d["Fu"]))
        D.append(e)
    fs = c(fs)
    reg, retries = dtype(xreg), 0
    while True:
        ok = True
        K, k, Qu, Quuk = [None] * T, [None] * T, [None] * T, [None] * T
        Vxx, Vx = D[T]["Lxx"].copy(), D[T]["Lx"].copy()
        if mut != "no_xreg":
            Vxx[np.diag_indices(NDX)] += reg
        if not feasible and mut != "no_gap_term":
            Vx = Vx + _mv(Vxx, fs[T])
        for t in range(T - 1, -1, -1):
            d = D[t]
            FxTV = _mm(d["Fx"].T, Vxx)
            Qxx = d["Lxx"] + _mm(FxTV, d["Fx"])
            Qx = d["Lx"] + _mv(d["Fx"].T, Vx)
            Qxu = _mm(FxTV, d["Fu"])
            Quu = d["Luu"] + _mm(_mm(d["Fu"].T, Vxx), d["Fu"])
            Qu[t] = d["Lu"] + _mv(d["Fu"].T, Vx)
            Quu[np.diag_indices(NV)] += reg
            L = cholesky_lower(Quu)
            if L is None:
                ok = False
                break
            K[t] = _solve_llt(L, Qxu.T)
            k[t] = _solve_llt(L, Qu[t])
            Quuk[t] = _mv(Quu, k[t])
            Vx = Qx - _mv(K[t].T, Qu[t])
            Vxx = Qxx - _mm(Qxu, K[t])
            if mut != "no_symmetrise":
                Vxx = (Vxx + Vxx.T) / 2
            if mut != "no_xreg":
                Vxx[np.diag_indices(NDX)] += reg
            if not feasible and mut != "no_gap_term":
                Vx = Vx + _mv(Vxx, fs[t])
            if not (np.isfinite(Vx).all() and np.isfinite(Vxx).all()):
                ok = False
                break
        if ok:
            break
        reg = min(reg * 10, dtype(reg_max))
        retries += 1
        if reg == reg_max:
            return dict(K=None, k=None, d1=None, d2=None, stop=None, reg=float(reg), retries=retries, gave_up=True)
    d1 = sum((np.dot(Qu[t], k[t]) for t in range(T)), dtype(0))
    d2 = -sum((np.dot(k[t], Quuk[t]) for t in range(T)), dtype(0))
    stop = sum((np.dot(Qu[t], Qu[t]) for t in range(T)), dtype(0))
    return dict(K=np.array(K), k=np.array(k), d1=d1, d2=d2, stop=stop, reg=float(reg), retries=retries, gave_up=False)


def riccati_errors(got, ref):
    """the comparison of a Riccati pass (a kernel's, float64's) with the long-double reference, per problem: normwise per node for the
    gains (max |got - ref| over max |ref| of that node, the largest node reported), relative for the three scalars"""
    f = lambda a: np.asarray(a, dtype=np.longdouble)           # noqa: E731
    out = {}
    for name in ("K", "k"):
        g, r = f(got[name]), f(ref[name])
        T = r.shape[0]
        den = np.abs(r).reshape(T, -1).max(axis=1)
        den = np.where(den > 0, den, 1)
        out[name] = float((np.abs(g - r).reshape(T, -1).max(axis=1) / den).max())
    for name in ("d1", "d2", "stop"):
        r = f(ref[name])
        out[name] = float(abs(f(got[name]) - r) / (abs(r) if r != 0 else 1))
    return out


RICCATI_QUANTITIES = ("K", "k", "d1", "d2", "stop")


def riccati_bounds(data, fs, xreg, feasible):
    """(long-double reference, float64 run, bound per quantity = 10 x the deviation of the float64 run from the reference): the
    yardstick of the kernels' Riccati pass on these inputs"""
    ref = riccati(data, fs, xreg, feasible, np.longdouble)
    f64 = riccati(data, fs, xreg, feasible, np.float64)
    if ref["gave_up"] or f64["gave_up"]:
        return ref, f64, None
    dev = riccati_errors(f64, ref)
    return ref, f64, {q: 10.0 * dev[q] for q in RICCATI_QUANTITIES}


# ------------------------------------------------------------------------------- the cases ---
def load_model(robot):
    """"solo12" / "go2": the committed models; "skew", "skew_axes", "skew_one", "skew_absorbed": the robots of tests/skew_robot.py with
    rotated joint placements / oblique axes, and the first of them with its placements folded into the child frames"""
    if robot.startswith("skew"):
        from tests import skew_robot
        return skew_robot.robot(robot)
    return urdf_model.RobotModel.from_json(open(os.path.join(ROBOTS, robot + ".json")).read())


def frame_groups(model):
    """frame ids on the feet (the last frame of each leg's last body), on a mid-leg body, on the base"""
    body = [f[0] for f in model.frames.values()]
    last = lambda b: max(i for i, bb in enumerate(body) if bb == b)        # noqa: E731
    feet = [last(b) for b in (3, 6, 9, 12)]
    mid = [last(b) for b in (2, 5, 8, 11)] + [last(b) for b in (1, 4, 7, 10)]
    base = [i for i, bb in enumerate(body) if bb == 0]
    return feet, mid, base


def _rand_rot(rng, angle):
    ax = rng.standard_normal(3)
    return rb.exp3(angle * ax / np.linalg.norm(ax))


class Case:
    """one batch of B problems over T nodes + the trajectory (xs, us) the passes are evaluated at"""

    def __init__(self, name, robot, seed, B, T, angle, weights="shared", vel=1.0, feasible=0, xreg=1e-9, indefinite=False, np_every=1):
        self.name, self.robot, self.B, self.T, self.angle, self.weights = name, robot, B, T, angle, weights
        self.feasible, self.xreg, self.indefinite, self.np_every = feasible, xreg, indefinite, np_every
        self.model = model = load_model(robot)
        rng = np.random.default_rng(seed)
        nn = T + 1
        feet, mid, base = frame_groups(model)
        nfr = len(model.frames)
        # ---- regularisation vectors: shared / per problem / per node.  state weights: zeros on base x, y as in the harness; the
        # velocity weights and the control weights stay positive (a node without control cost then still has a definite Q_uu)
        nb = 1 if weights == "shared" else B
        nt = nn if weights == "node" else 1
        sw = np.exp(rng.uniform(np.log(0.5), np.log(1e3), (nb, nt, NDX)))
        sw[:, :, 0:2] = 0.0
        sw[:, :, NV:] = np.exp(rng.uniform(np.log(0.5), np.log(1e2), (nb, nt, NV)))
        cw = np.exp(rng.uniform(np.log(1.0), np.log(1e3), (nb, max(nt - 1, 1), NV)))      # ctrl_w has no terminal row
        if indefinite:                     # test_riccati_pass_that_fails_and_restarts: leg joint velocities rewarded instead of penalised
            sw[:, :, 24:30] = -40.0
        # x_reg: a reference per problem (per node in "node"), base orientation away from the identity
        xr = np.zeros((B, nt, NX))
        Rreg = np.zeros((B, nt, 3, 3))
        for b in range(B):
            for t in range(nt):
                Rreg[b, t] = _rand_rot(rng, 0.7)
                xr[b, t, 0:3] = rng.uniform(-0.3, 0.3, 3) + [0, 0, 0.3]
                xr[b, t, 3:7] = rb.R_to_quat(Rreg[b, t])
                xr[b, t, 7:NQ] = rng.uniform(-1.0, 1.0, 12)
                xr[b, t, NQ:] = 0.2 * rng.standard_normal(NV)
        self.state_w, self.ctrl_w, self.x_reg = (sw, cw, xr) if weights == "node" else (sw[:, 0], cw[:, 0], xr[:, 0])
        # ---- trajectory: base orientation = x_reg's turned by `angle` about a random axis, q and -q alternating; joints in +-pi
        xs = np.zeros((B, nn, NX))
        for b in range(B):
            for t in range(nn):
                R = Rreg[b, t if weights == "node" else 0] @ _rand_rot(rng, angle)
                q = rb.R_to_quat(R)
                xs[b, t, 0:3] = rng.uniform(-0.5, 0.5, 3) + [0, 0, 0.3]
                xs[b, t, 3:7] = -q if (b + t) % 2 else q
                xs[b, t, 7:NQ] = rng.uniform(-np.pi, np.pi, 12)
                xs[b, t, NQ:] = vel * rng.standard_normal(NV)
        self.xs, self.us = xs, rng.standard_normal((B, T, NV))
        self.x0 = np.array([rb.state_integrate(model, xs[b, 0], 0.1 * rng.standard_normal(NDX)) for b in range(B)])
        self.dt = rng.uniform(0.01, 0.1, (B, T))
        # ---- tasks.  node pattern p = (t + b) % 5: 0 everything on, four different frames (foot, mid-leg, base, any);
        # 1 no control cost, slots 1 and 3 off; 2 no CoM and no momentum cost, slots 0 and 2 name the same frame; 3 no state cost, all
        # slots off; 4 everything on, slots 0 and 1 the same frame with different weights and references.  (Pattern 1 is followed by
        # pattern 2, whose state cost keeps Q_uu of the node without control cost definite.)
        tk = np.zeros((B, nn, NTASK))
        for b in range(B):
            for t in range(nn):
                p = (t + b) % 5
                fr = [feet[rng.integers(4)], mid[rng.integers(len(mid))], base[rng.integers(len(base))], int(rng.integers(nfr))]
                w = [1e4, 1e3, 37.5, 1e4 * rng.uniform(0.1, 1.0)]
                if p == 1:
                    w[1] = w[3] = 0.0
                elif p == 2:
                    fr[2] = fr[0]
                elif p == 3:
                    w = [0.0] * 4
                elif p == 4:
                    fr[1] = fr[0]
                for s in range(4):
                    tk[b, t, 5 * s] = w[s]
                    tk[b, t, 5 * s + 1] = fr[s]
                    tk[b, t, 5 * s + 2:5 * s + 5] = rng.uniform(-0.5, 0.5, 3)
                tk[b, t, 20] = 0.0 if p == 2 else 1e2 * rng.uniform(0.5, 2.0)
                tk[b, t, 21:24] = rng.uniform(-0.3, 0.3, 3) + [0, 0, 0.3]
                tk[b, t, 24] = 0.0 if p == 2 else 5e2
                tk[b, t, 25:31] = rng.standard_normal(6)
                tk[b, t, 31] = 0.0 if p == 3 else 5e-2
                tk[b, t, 32] = 0.0 if p == 1 else 1e-5
        self.tasks = tk

    # the regularisation vectors of node t of problem b
    def node_weights(self, b, t):
        bb = 0 if self.state_w.shape[0] == 1 else b
        if self.weights == "node":
            return self.state_w[bb, t], self.x_reg[b, t], self.ctrl_w[bb, min(t, self.T - 1)]
        return self.state_w[bb], self.x_reg[b], self.ctrl_w[bb]

    def np_nodes(self):
        """(b, t) the numpy twin is evaluated at: every node of a small case, every np_every-th of a large one"""
        return [(i // (self.T + 1), i % (self.T + 1)) for i in range(0, self.B * (self.T + 1), self.np_every)]

    def np_problem(self, b, tasks=None):
        model, names = self.model, list(self.model.frames)
        prob = ik_ddp_np.IKProblem(model, self.T)
        tk_all = self.tasks if tasks is None else tasks
        for t in range(self.T + 1):
            tk = tk_all[b, t]
            sw, xr, cw = self.node_weights(b, t)
            for s in range(4):
                if tk[5 * s] != 0:
                    prob._add(t, "f%d" % s, ("frame", tk[5 * s], (names[int(tk[5 * s + 1])], tk[5 * s + 2:5 * s + 5])))
            prob._add(t, "com", ("com", tk[20], tk[21:24]))
            prob._add(t, "mom", ("mom", tk[24], tk[25:31]))
            prob._add(t, "x", ("state", tk[31], (sw, xr)))
            prob._add(t, "u", ("ctrl", tk[32], cw))
        prob.setup_costs(self.dt[b])
        return prob


def cases(which="all"):
    """the fixed case set.  Horizons 1, 2, 7, 10, 64 (even and odd node counts), base orientation 0 .. 3.0 rad away from x_reg's,
    both robots and the skewed test robots (tests/skew_robot.py), the three weight layouts, both feasibility flags and regularisations,
    velocity scales 1 and 10; one case whose Q_uu is indefinite until the regularisation has grown; one of 256 problems (1536 node
    pairs: the one-wave derivative kernel's own launch size)."""
    small = [
        Case("solo12_T1_a0_shared", "solo12", 101, 5, 1, 0.0, "shared", 1.0, 0, 1e-9),
        Case("solo12_T2_a1e-9_problem_feas_xreg1", "solo12", 102, 5, 2, 1e-9, "problem", 10.0, 1, 1.0),
        Case("go2_T7_a1e-4_node_xreg1", "go2", 103, 5, 7, 1e-4, "node", 1.0, 0, 1.0),
        Case("solo12_T10_a0.5_node_vel10", "solo12", 104, 5, 10, 0.5, "node", 10.0, 0, 1e-9),
        Case("go2_T10_a1.57_shared_feas", "go2", 105, 5, 10, np.pi / 2, "shared", 1.0, 1, 1e-9),
        Case("solo12_T7_a3.0_problem", "solo12", 106, 5, 7, 3.0, "problem", 1.0, 0, 1e-9),
        Case("go2_T2_a3.0_shared_xreg1", "go2", 107, 5, 2, 3.0, "shared", 10.0, 0, 1.0),
        Case("go2_T1_a1e-4_node_feas", "go2", 108, 5, 1, 1e-4, "node", 1.0, 1, 1e-9),
        Case("solo12_T10_indefinite", "solo12", 109, 5, 10, 0.5, "shared", 1.0, 0, 1e-9, indefinite=True),
    ]
    # rotated joint placements and oblique axes (tests/skew_robot.py; compared pairwise in tests/test_skew_robot_gpu.py).  The absorbed
    # case takes the seed of the skew case of its name: identical xs, us, tasks and weights on the kinematically identical robot
    small += [
        Case("skew_T1_a0_shared", "skew", 121, 5, 1, 0.0, "shared", 1.0, 0, 1e-9),
        Case("skew_T7_a1.57_node_feas_xreg1", "skew", 122, 5, 7, np.pi / 2, "node", 10.0, 1, 1.0),
        Case("skew_axes_T2_a3.0_problem", "skew_axes", 123, 5, 2, 3.0, "problem", 1.0, 0, 1e-9),
        Case("skew_one_T7_a0.5_shared", "skew_one", 124, 5, 7, 0.5, "shared", 1.0, 0, 1e-9),
        Case("skew_absorbed_T7_a1.57_node_feas_xreg1", "skew_absorbed", 122, 5, 7, np.pi / 2, "node", 10.0, 1, 1.0),
    ]
    if which == "small":
        return small
    long_ = [
        Case("go2_T64_a0.5_problem", "go2", 110, 5, 64, 0.5, "problem", 1.0, 0, 1e-9),
        Case("solo12_T64_a1.57_node_feas_xreg1", "solo12", 111, 5, 64, np.pi / 2, "node", 10.0, 1, 1.0),
    ]
    if which == "no_big":
        return small + long_
    return small + long_ + [Case("solo12_B256_T10_a0.5_shared", "solo12", 112, 256, 10, 0.5, "shared", 1.0, 0, 1e-9, np_every=16)]


# ------------------------------------------------------------------- the twins on a case ---
DERIV_QUANTITIES = ("cost", "xnext", "Fx", "Fu", "Lx", "Lxx", "Lu", "Luu", "fs")
# the bounds tests/test_ik_twin_cpu.py holds the two twins to at node level (test_node_derivatives_agree,
# test_state_operators_and_se3_jacobians for the state difference): the floor under 10 x their measured gap
FLOOR = dict(cost=1e-13, xnext=1e-14, Fx=1e-12, Fu=1e-12, Lx=1e-12, Lxx=1e-12, Lu=1e-13, Luu=1e-13, fs=1e-13)


def c_twin_node(cm, case, b, t):
    sw, xr, cw = case.node_weights(b, t)
    u = case.us[b, t] if t < case.T else None
    d = ic.node(cm, case.T, t, case.dt[b], case.tasks[b], sw, xr, cw, case.xs[b, t], u)
    if t == case.T:
        d = dict(cost=d["cost"], Lx=d["Lx"], Lxx=d["Lxx"])
    else:
        d["Luu"] = np.diag(d["Luu"]).copy()
    return d


def np_twin_node(prob, case, b, t):
    d = ik_ddp_np.node_calc(prob, t, case.xs[b, t], case.us[b, t] if t < case.T else None, diff=True)
    if t < case.T:
        assert np.count_nonzero(d["Luu"] - np.diag(np.diag(d["Luu"]))) == 0
        d["Luu"] = np.diag(d["Luu"]).copy()
    return d


def gaps_c(cm, case, xnext):
    """fs [B][T+1][36] by the compiled twin's state difference: node 0 against x0, node t + 1 against xnext of node t"""
    fs = np.zeros((case.B, case.T + 1, NDX))
    z = np.zeros(NDX)
    for b in range(case.B):
        for t in range(case.T + 1):
            fs[b, t] = ic.state_ops(cm, case.xs[b, t], case.x0[b] if t == 0 else xnext[b][t - 1], z)["diff"]
    return fs


def node_error(got, ref, q):
    """max |got - ref| over max |ref| of one quantity of one node (absolute where the reference is all zero)"""
    g, r = np.asarray(got[q], dtype=np.float64), np.asarray(ref[q], dtype=np.float64)
    if q == "xnext" and np.dot(g[3:7], r[3:7]) < 0:        # q and -q are one orientation: the twins return the canonical sign of
        g = g.copy()                                       # R_to_quat, the kernel keeps the sign of the state it integrates
        g[3:7] = -g[3:7]
    den = np.abs(r).max()
    return float(np.abs(g - r).max() / (den if den > 0 else 1.0))


def twins_on_case(case):
    """both CPU twins on a case: (C twin nodes [b][t], numpy twin nodes {(b, t)}, fs of each, gap per quantity = the largest
    node_error between them over the numpy twin's nodes, tolerance per quantity = max(10 x gap, FLOOR))"""
    cm = ic.Model(case.model)
    ref_c = [[c_twin_node(cm, case, b, t) for t in range(case.T + 1)] for b in range(case.B)]
    fs_c = gaps_c(cm, case, [[ref_c[b][t]["xnext"] for t in range(case.T)] for b in range(case.B)])
    ref_np, probs = {}, {}
    gap = {q: 0.0 for q in DERIV_QUANTITIES}
    for b, t in case.np_nodes():
        if b not in probs:
            probs[b] = case.np_problem(b)
        d = ref_np[(b, t)] = np_twin_node(probs[b], case, b, t)
        # (the numpy twin's gap of this node needs its xnext of the node before: taken from the C twin where that node was not sampled)
        prev = case.x0[b] if t == 0 else (ref_np[(b, t - 1)]["xnext"] if (b, t - 1) in ref_np else ref_c[b][t - 1]["xnext"])
        d["fs"] = rb.state_diff(case.model, case.xs[b, t], prev)
        cnode = dict(ref_c[b][t], fs=fs_c[b, t])
        for q in DERIV_QUANTITIES:
            if q in d and q in cnode:
                gap[q] = max(gap[q], node_error(cnode, d, q))
    tol = {q: max(10.0 * gap[q], FLOOR[q]) for q in DERIV_QUANTITIES}
    return dict(c=ref_c, fs_c=fs_c, np=ref_np, gap=gap, tol=tol)


def deriv_errors(case, got, fs_got, tw):
    """the derivative-pass comparison: got[b][t] (dicts as unpack_node gives them + cost) and fs_got [B][T+1][36] against the C twin at
    every node and the numpy twin at its sample; returns {quantity: (largest node_error, (b, t, twin))}.  A feasible case expects
    fs == 0 exactly (error inf otherwise)."""
    worst = {q: (0.0, None) for q in DERIV_QUANTITIES}

    def note(q, e, where):
        if worst[q][1] is None or e > worst[q][0]:
            worst[q] = (e, where)

    for b in range(case.B):
        for t in range(case.T + 1):
            g = dict(got[b][t], fs=fs_got[b, t])
            refs = [("c", dict(tw["c"][b][t], fs=tw["fs_c"][b, t]))] + ([("np", tw["np"][(b, t)])] if (b, t) in tw["np"] else [])
            for name, r in refs:
                for q in DERIV_QUANTITIES:
                    if q == "fs" and case.feasible:
                        note(q, 0.0 if not np.any(g["fs"]) else np.inf, (b, t, "zero"))
                    elif q in r:
                        note(q, node_error(g, r, q), (b, t, name))
    return worst


# -------------------------------------------------------- single-term mutations of the references ---
@contextlib.contextmanager
def mutated_twin(kind):
    """the numpy twin with one term wrong (tests/test_ik_passes_cpu.py: the comparison must notice each of them)"""
    saved = (rb.state_jdiff_second, rb.Kin.frame_jacobian_lin, rb.Kin.dh_dq)
    try:
        if kind == "jlog6_identity":
            rb.state_jdiff_second = lambda model, x0, x1: np.eye(2 * model.nv)
        elif kind == "frame_jacobian_at_parent":
            orig = saved[1]

            def at_parent(self, name):
                J = orig(self, name)
                b = self.model.frames[name][0]
                if b > 0:
                    J[:, self.support[b][-1]] = 0.0            # the frame's own joint does not move it
                return J
            rb.Kin.frame_jacobian_lin = at_parent
        elif kind == "momentum_without_dh_dq":
            orig_dh = saved[2]
            rb.Kin.dh_dq = lambda self: 0.0 * orig_dh(self)
        else:
            raise KeyError(kind)
        yield
    finally:
        rb.state_jdiff_second, rb.Kin.frame_jacobian_lin, rb.Kin.dh_dq = saved
