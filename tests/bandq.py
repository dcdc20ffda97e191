"""Shared pieces of the band-cost tests (costs between neighbouring knots): the inputs the issue fixes and the CPU restatement's call."""
import numpy as np

from bunmpc_amd import problems
from tests import blockq_np

LX = np.array([2.25e6, 1e4, 1e5, 3e5, 2.25e6, 5e4])      # tests/test_block_cost_gpu.py's step constants: retries in both loops
LF = np.array([506.25, 10.0, 50.0, 506.25, 20.0, 100.0])
MAIN = (0.5, 0.5)        # (lam_f, lam_x) of the main parity test
STRONG = (4.0, 2.0)      # ... of the strong-weights test: cold starts backtrack twice in the force loop


def case(oracle, config, B, H=None, lam=MAIN, sides="xf"):
    """batch, its diagonal raw arrays, the rate costs (problems.rate_costs) and the raw dict for solve_host; a side not in `sides`
    keeps the batch's own diagonal and gets no coupling"""
    b = problems.make_batch(config, B, H=H) if H else problems.make_batch(config, B)
    pre = oracle.solve_batch(b, num_iters=0)
    rc = problems.rate_costs(pre["Qx"], pre["Qf"], b.E, lam_x=lam[1], lam_f=lam[0])
    raw = dict(Qx=pre["Qx"], qx=pre["qx"], lbx=pre["lbx"], ubx=pre["ubx"], Qf=pre["Qf"])
    if "x" in sides:
        raw.update(Qx=rc["Qx"], Qx_off=rc["Qx_off"])
    if "f" in sides:
        raw.update(Qf=rc["Qf"], Qf_off=rc["Qf_off"])
    return b, pre, rc, raw


def matrices(raw, i, E):
    """problem i's dense Q_x and Q_f as set_cost_x / set_cost_f take them"""
    H = raw["Qf"].shape[1] // (3 * E)
    Qx = problems.band_matrix(raw["Qx"][i], raw["Qx_off"][i]) if "Qx_off" in raw else np.diag(raw["Qx"][i])
    if "Qf_off" in raw and H > 1:
        Qf = problems.band_matrix(raw["Qf"][i], raw["Qf_off"][i])
    else:
        Qf = np.diag(raw["Qf"][i])
    return Qx, Qf


def restatement(b, i, raw, iters, warm=None, L_x=2.25e6, L_f=506.25, sparse=True):
    """problem i through tests/blockq_np.py (the reference's ProblemData with the whole matrix), cold or from warm = (X, F, P)"""
    X0, F0, P0 = b.warm_start() if warm is None else warm
    Qx, Qf = matrices(raw, i, b.E)
    return blockq_np.biconvex_solve(b.cnt_plan[i], b.dt[i], b.m, b.x_init[i], Qx, raw["qx"][i], Qf, raw["lbx"][i], raw["ubx"][i],
                                    X0[i], F0[i], P0[i], sparse=sparse, L_x=L_x, L_f=L_f, rho=b.rho, mu=b.mu, num_iters=iters)
