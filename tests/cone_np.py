"""The CPU twin of the Euclidean friction-cone projection (bmpc_cone_t, projection 1) and the shared pieces of its tests: the projection
itself, the numpy restatement of the solve with it (oracle/oracle_np.py, which takes the force FISTA's projection as an argument), and
the cases the CPU and the GPU tests run."""
import functools

import numpy as np

from bunmpc_amd import problems
from oracle import oracle_np
from tests import util

CONFIGS = ["solo12_trot", "biped_walk"]
L_F = 40.0                  # the force step constant the cases start from: every case takes force-loop retries
MU_RANGE = (0.05, 0.3)


def project(v, mu, count=None):
    """Nearest point of the cone |f_xy| <= mu f_z for every 3-vector of v (any shape whose size is a multiple of 3), mu a scalar or one
    coefficient per vector.  Branch tests on squared quantities; the square root and the divisions on the third branch only.
    count: a list of three ints, increased by the vectors on the zero / inside / surface branch."""
    y = np.array(v, dtype=np.float64).reshape(-1, 3)
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64).reshape(-1), (y.shape[0],))
    fx, fy, fz = y[:, 0], y[:, 1], y[:, 2]
    s2 = fx * fx + fy * fy
    mu2 = mu * mu
    zero = (fz <= 0) & (mu2 * s2 <= fz * fz)                      # the polar cone; wins at the origin
    inside = ~zero & (fz >= 0) & (s2 <= mu2 * (fz * fz))
    surf = ~zero & ~inside
    out = y.copy()
    out[zero] = 0.0
    s = np.sqrt(s2[surf])
    t = (mu[surf] * s + fz[surf]) / (mu2[surf] + 1.0)
    k = mu[surf] * t / s
    out[surf, 0] = fx[surf] * k
    out[surf, 1] = fy[surf] * k
    out[surf, 2] = t
    if count is not None:
        count[0] += int(zero.sum()); count[1] += int(inside.sum()); count[2] += int(surf.sum())
    return out.reshape(np.shape(v))


def raw_of(b, i):
    """problem i's raw cost and bound arrays, as create_cost_X / create_cost_F / create_bound_constraints leave them"""
    def row(a):
        return a[0] if a.shape[0] == 1 else a[i]
    Qx, qx = oracle_np.create_cost_X(row(b.W_X), row(b.W_X_ter), b.X_ter[i], b.X_nom[i])
    lbx, ubx = oracle_np.create_bound_constraints(b.cnt_plan[i], row(b.bounds))
    return dict(Qx=Qx, qx=qx, Qf=np.array(row(b.W_F)), lbx=lbx, ubx=ubx)


def raw_batch(b):
    """... of every problem, stacked: the raw= dict of batch.solve_host"""
    rows = [raw_of(b, i) for i in range(b.B)]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def restatement(b, i, iters, mu, projection=project, **kw):
    """problem i of batch b through util.restatement with `projection` (v, mu, count) applied by the force FISTA.  mu: a scalar or (H, E);
    kw: util.restatement's.  Beside biconvex_solve's result: "branches", the vectors that took the zero / inside / surface branch over
    the whole solve."""
    count = [0, 0, 0]
    mu = np.asarray(mu, dtype=np.float64)
    out = util.restatement(b, i, {k: {i: v} for k, v in raw_of(b, i).items()}, iters, mu=float(mu) if mu.ndim == 0 else mu.reshape(-1),
                           projection=lambda v, m: projection(v, m, count), **kw)
    out["branches"] = np.array(count)
    return out


def one_ulp(x_init):
    """x_init with its first component moved up by one ulp"""
    x = np.array(x_init, dtype=np.float64)
    x[0] = np.nextafter(x[0], np.inf)
    return x


@functools.lru_cache(maxsize=None)
def case(config, H):
    """(batch of six problems, mu (6, H, E) ~ U[0.05, 0.3], warm = (X = tile(x_init), F ~ N((0, 0, 3), 4^2) per foot, P = 0), iters):
    fixed seed per (H, E); the solve starts from L_f = 40 and the constructor's L_x"""
    b = problems.make_batch(config, 6, H=H)
    rng = np.random.default_rng([20251017, H, b.E])
    mu = rng.uniform(MU_RANGE[0], MU_RANGE[1], size=(6, H, b.E))
    F = rng.normal(0.0, 4.0, size=(6, H, b.E, 3)) + np.array([0.0, 0.0, 3.0])
    X, _, P = b.warm_start()
    return b, mu, (X, F.reshape(6, -1), P), (1 if H == 63 else 3)


def linear_force_cost(b):
    """a small linear force cost qf (B, 3EH) for the raw form with qf, fixed per batch shape"""
    return np.random.default_rng([7, b.H, b.E]).normal(0.0, 0.05, size=(b.B, 3 * b.E * b.H))


@functools.lru_cache(maxsize=None)
def twin(config, H, perturbed=False, with_qf=False):
    """the restatement of every problem of case(config, H), computed once per process (the results are shared: do not modify them);
    perturbed: x_init[0] of every problem moved by one ulp"""
    b, mu, warm, iters = case(config, H)
    qf = linear_force_cost(b) if with_qf else None
    return [restatement(b, i, iters, mu[i], warm=warm, L_f=L_F, x_init=one_ulp(b.x_init[i]) if perturbed else None,
                        qf=None if qf is None else qf[i]) for i in range(b.B)]
