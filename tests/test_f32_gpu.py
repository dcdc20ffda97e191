"""The fp32 centroidal kernels (biconvex_admm_kernel_f32<LPP, E>, precision = 1) against their mixed-precision CPU twin (tests/f32_np.py)
on the GPU (run with -m gpu): every case and regime of the twin's module through batch.solve_host(precision="f32") -- the dispatch, the
discrete path exactly, the values within K_SPREAD x the twin ensemble's own distance from the strict fp64 oracle, the projection set and
the reported violation -- then wave mates of a diverging problem, rows past B, and carried step constants.

tests/test_f32_cpu.py shows that the twin is fit to judge (every decision of every ensemble member is clear of its threshold and the
fp64 oracle takes the same path) and which faults the judgement catches."""
import numpy as np
import pytest

from bunmpc_amd import _lib
from bunmpc_amd import batch as bb
from tests import f32_np

pytestmark = pytest.mark.gpu
KERNEL = b"biconvex_admm_kernel_f32"
CASE_IDS = [f32_np.case_id(c) for c in f32_np.CASES]
OUT = ("X", "F", "P", "L_x", "L_f", "stats", "dyn_viol")


def _dispatched(hiplib, lanes):
    assert hiplib.bmpc_biconvex_last_kernel_name() == KERNEL
    assert hiplib.bmpc_biconvex_last_lanes_per_problem() == lanes


def _solve(hiplib, case, regime, b=None):
    b = f32_np.batch(case)[0] if b is None else b
    s = f32_np.settings(case, regime)
    got = bb.solve_host(b, num_iters=s["num_iters"], maxit=s["maxit"], tol=s["tol"], exit_tol=s["exit_tol"], warm=s["warm"], L_x=s["L_x"], L_f=s["L_f"],
                        precision="f32", keep_hist=True)
    _dispatched(hiplib, case[0])
    return got


def _judged(got, case, regime, oracle, tag, exact=True):
    """the discrete path exactly (the oracle's, which tests/test_f32_cpu.py shows to be every twin member's), the values and hist within
    K_SPREAD x max(y_i, 2^-23) of the oracle, y_i the largest distance of a member of problem i's twin ensemble from it"""
    ens, ref = f32_np.members(case, regime), f32_np.oracle_solve(oracle, case, regime)
    j = f32_np.judge(got, ens, ref, exact)
    print(tag, "worst error / y_i %.2f (hist %.2f); error %s y %s path %s" % (j["ratio"].max(), j["ratio_hist"].max(), j["err"], j["y"], j["path"].tolist()))
    cols = slice(None) if exact else [0, 3, 4, 5]      # (regime r: ADMM count, retry counts, status)
    for r in ens[:1] + [ref]:
        if exact:
            assert np.array_equal(got["trace"], r["trace"]), (got["trace"].tolist(), r["trace"].tolist())
        assert np.array_equal(got["stats"][:, cols], r["stats"][:, cols]), (got["stats"].tolist(), r["stats"].tolist())
        assert np.array_equal(got["L_x"], r["L_x"]) and np.array_equal(got["L_f"], r["L_f"])
    assert np.all(j["err"] <= j["bound"]), (j["err"], j["bound"])
    assert np.all(j["err_hist"] <= j["bound_hist"]), (j["err_hist"], j["bound_hist"])
    return j


@pytest.mark.parametrize("regime", f32_np.REGIMES)
@pytest.mark.parametrize("case", f32_np.CASES, ids=CASE_IDS)
def test_kernel_against_the_twin(hiplib, oracle, case, regime):
    b = f32_np.batch(case)[0]
    got = _solve(hiplib, case, regime)
    _judged(got, case, regime, oracle, "%s %s" % (f32_np.case_id(case), regime))
    # the projection set: the projection is the last thing applied to F -- fz >= 0, and swing feet exactly 0.  (Regime b starts from random
    # forces on every foot: a swing foot's force only shrinks by 1 - 2 w / L per iteration, in the reference as here, so there the
    # forces that are exactly 0 are the oracle's zeros.)
    F = got["F"].reshape(b.B, b.H, b.E, 3)
    assert np.all(F[..., 2] >= 0)
    assert np.all(got["F"][f32_np.oracle_solve(oracle, case, regime)["F"] == 0.0] == 0.0)
    if regime != "b":
        assert np.all(F[b.cnt_plan[..., 0] == 0] == 0.0)
    # the violation the kernel reports, re-derived in fp64 from the returned X, F
    for i in range(b.B):
        A, bf = oracle.dense_A_f(b.cnt_plan[i], b.dt[i], b.m, got["F"][i], b.x_init[i])
        r = np.linalg.norm(A @ got["X"][i] - bf)
        assert abs(r - got["dyn_viol"][i]) <= 1e-4 * max(r, 1e-3), (i, r, got["dyn_viol"][i])
        assert got["dyn_viol"][i] == got["hist"][i, got["stats"][i, 0] - 1]


@pytest.mark.parametrize("case", f32_np.R_CASES, ids=[f32_np.case_id(c) for c in f32_np.R_CASES])
def test_retry_decisions_at_the_reference_tolerances(hiplib, oracle, case):
    """Regime r of tests/f32_np.py: steps of a few fp32 ulp, where the force step's retry test must take A d from d.  The retry counts,
    the ADMM count, the status and the returned step constants are the oracle's and every twin member's; the values within K_SPREAD x
    max(y_i, 1e-5)."""
    got = _solve(hiplib, case, "r")
    _judged(got, case, "r", oracle, "%s r" % f32_np.case_id(case), exact=False)
    assert np.all(np.isfinite(got["L_f"])) and np.all(got["stats"][:, 3] <= 1)


@pytest.mark.parametrize("magnitude", [1e30, 1e38])
@pytest.mark.parametrize("case", [(16, 15, 6, "biped_walk"), (32, 20, 5, "solo12_trot")], ids=["16-15-biped_walk", "32-20-solo12_trot"])
def test_wave_mates_of_a_diverging_problem(hiplib, case, magnitude):
    """Problem 1 of the first wave has x_init and X_nom at `magnitude`.  Every output bit of the other problems equals the run without
    it, and through the device entry point nothing is written past row B of any output.  What the problem itself returns is the twin's
    prediction: at 1e38 fp32 overflows at once, the violation is NaN and the status 2; at 1e30 the products stay finite -- the force
    loop's retry test fires until L_f itself is +inf (204 retries from 506.25), the forces freeze and the solve ends with status 0."""
    import dataclasses
    import torch
    assert case in f32_np.CASES
    b, s = f32_np.batch(case)[0], f32_np.settings(case, "a")
    want = _solve(hiplib, case, "a")
    x_init, X_nom = b.x_init.copy(), b.X_nom.copy()
    x_init[1], X_nom[1] = magnitude, magnitude
    bad = dataclasses.replace(b, x_init=x_init, X_nom=X_nom)
    with np.errstate(all="ignore"):
        twin = f32_np.solve(bad, num_iters=s["num_iters"], maxit=s["maxit"], tol=s["tol"], exit_tol=s["exit_tol"])
    got = _solve(hiplib, case, "a", bad)
    others = np.arange(b.B) != 1
    print(case, magnitude, "stats", got["stats"][1].tolist(), "twin", twin["stats"][1].tolist(), "L_f", got["L_f"][1], "hist", got["hist"][1])
    assert np.array_equal(got["stats"][1], twin["stats"][1]) and got["L_f"][1] == twin["L_f"][1]
    assert got["stats"][1, 5] == (2 if magnitude == 1e38 else 0) and np.all(got["stats"][others, 5] == 0)
    for k in OUT + ("hist", "trace"):
        assert np.array_equal(got[k][others], want[k][others]), k
    # the device entry point, its output arrays one problem longer than B and filled with sentinels
    dev = bb.DeviceBatch(bad, device="cuda:0", num_iters=s["num_iters"], maxit=s["maxit"], tol=s["tol"], exit_tol=s["exit_tol"], precision="f32")
    for name in ("X", "F", "P", "L_x", "L_f", "dyn_viol", "stats"):
        t = getattr(dev, name)
        longer = torch.full((t.shape[0] + 1,) + tuple(t.shape[1:]), -77, dtype=t.dtype, device=t.device)
        setattr(dev, name, longer)
        setattr(dev.desc, name, longer.data_ptr())
    dev.solve()
    res = dev.results()
    _dispatched(hiplib, case[0])
    for k in OUT:
        assert np.array_equal(res[k][:b.B][others], want[k][others]), k
        assert np.all(res[k][b.B] == -77), k
    assert np.array_equal(res["stats"][1], got["stats"][1])


def test_carried_step_constants(hiplib, oracle):
    """cold_start = 2 keeps the arrays' L_f (40: the force loop backtracks from there); cold_start = 1 then resets it to BMPC_L0_F"""
    case = (32, 20, 5, "solo12_trot")
    assert case in f32_np.CASES
    b, s = f32_np.batch(case)[0], f32_np.settings(case, "k")
    dev = bb.DeviceBatch(b, device="cuda:0", num_iters=s["num_iters"], maxit=s["maxit"], tol=s["tol"], exit_tol=s["exit_tol"], precision="f32", keep_hist=True)
    dev.set_step_constants(s["L_x"], s["L_f"])
    dev.cold_start(carry_step_constants=True)
    dev.solve()
    got = dev.results()
    _dispatched(hiplib, case[0])
    j = _judged(got, case, "k", oracle, "carried (cold_start = 2)")
    assert np.all(got["stats"][:, 3] > 0) and np.all(got["L_f"] > f32_np.L_F_RETRY) and np.all(got["L_f"] != _lib.L0_F)
    dev.cold_start(carry_step_constants=False)      # the arrays now hold what that solve left
    dev.solve()
    got = dev.results()
    _dispatched(hiplib, case[0])
    _judged(got, case, "a", oracle, "reset (cold_start = 1)")
    assert np.all(got["L_f"] == _lib.L0_F * 1.5 ** got["stats"][:, 3])
    assert j["path"].all()
