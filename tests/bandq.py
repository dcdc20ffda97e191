"""Shared pieces of the band-cost tests (costs between neighbouring knots): the inputs the issue fixes and the CPU restatement's call."""
import numpy as np

from bunmpc_amd import problems
from tests import blockq_np, util

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


def restatement(b, i, raw, iters, sparse=True, **kw):
    """problem i through tests/blockq_np.py (the reference's ProblemData with the whole matrix); kw: util.restatement's"""
    Qx, Qf = matrices(raw, i, b.E)
    return util.restatement(b, i, dict(raw, Qx={i: Qx}, Qf={i: Qf}), iters, problem=blockq_np.PROBLEM[sparse], **kw)
