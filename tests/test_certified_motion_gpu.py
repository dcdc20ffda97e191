"""The motion step's certificate in the benchmark's kernel (biconvex_admm_kernel<double, 32, 4, false, false, 2>):
a motion phase whose Hessian bound is below (L/2)(1 - eta) runs its FISTA loop without the backtracking test.  The test cannot fire
there, so bmpc_set_certified_steps 0 (off), 1 (both steps) and 2 (force step only) must not show in any output, bit for bit and
NaN-aware; the telemetry (bmpc_batch_t.cert_phases) says which phases ran certified, and is held to the numpy restatement of the
bound (tools/certify_rate.py)."""
import os
import sys

import numpy as np
import pytest

from bunmpc_amd import batch as bb
from bunmpc_amd import problems
from tests.util import TOL_FP64 as TOL, knob_setter, launch_record, rel_l2      # TOL: what tests/test_biconvex_gpu.py holds solo12_trot to

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import certify_rate as cr  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("X", "F", "P", "L_x", "L_f", "stats", "trace", "hist", "dyn_viol")
HEADLINE = ("biconvex_admm_kernel", 32, 2)


@pytest.fixture
def knobs():
    """sets dispatch knobs for one test and restores every one of them afterwards; the headline kernel is forced for every launch"""
    with knob_setter() as set_:
        set_("bmpc_set_latency_mapping_max_batch", 0)
        set_("bmpc_set_three_per_wave", 0)
        set_("bmpc_set_two_waves_per_simd", 1)
        yield set_


def _switches(knobs, hiplib, solve, values=(0, 1, 2)):
    """solve() under every value of the switch: the headline kernel each time, every output equal to the first value's"""
    out = {}
    for v in values:
        knobs("bmpc_set_certified_steps", v)
        out[v] = solve()
        assert launch_record(hiplib) == HEADLINE
    for v in values[1:]:
        for k in KEYS:
            assert np.array_equal(out[values[0]][k], out[v][k], equal_nan=True), (v, k)
    return out


def test_cold_and_warm_starts(hiplib, knobs):
    """five problems (the last wave holds one problem and one padding segment): a cold start, then a warm start from its results with
    the step constants it left behind"""
    b = problems.make_batch("solo12_trot", 5)
    cold = _switches(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, keep_hist=True, cert_phases=True))
    assert np.all(cold[1]["stats"][:, 0] == 10)
    assert np.array_equal(cold[1]["cert_phases"], np.full((5, 2), 10))
    assert np.array_equal(cold[2]["cert_phases"], np.stack([np.full(5, 10), np.zeros(5, int)], axis=1))
    assert np.array_equal(cold[0]["cert_phases"], np.zeros((5, 2), int))
    c = cold[1]
    warm = _switches(knobs, hiplib, lambda: bb.solve_host(b, num_iters=4, warm=(c["X"], c["F"], c["P"]), L_x=c["L_x"], L_f=c["L_f"],
                                                         keep_hist=True, cert_phases=True))
    assert np.all(warm[2]["cert_phases"][:, 1] == 0) and np.all(warm[0]["cert_phases"] == 0)
    assert np.all(warm[1]["cert_phases"] <= warm[1]["stats"][:, :1]) and np.array_equal(warm[1]["cert_phases"][:, 0], warm[2]["cert_phases"][:, 0])


def test_oracle_comparison(hiplib, knobs, oracle):
    """the same five problems against the strict CPU oracle: the discrete path per ADMM iteration, X and F"""
    b = problems.make_batch("solo12_trot", 5)
    ref = oracle.solve_batch(b, num_iters=10, trace=True)
    got = _switches(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, keep_hist=True), values=(1,))[1]
    assert np.array_equal(got["trace"], ref["trace"])
    for k in ("X", "F"):
        err = rel_l2(got[k], ref[k])
        print(k, "rel-L2 against the oracle", err)
        assert np.all(err < TOL), (k, err)


def test_small_step_constants(hiplib, knobs, oracle):
    """L_x far below the Hessian's bound on every third problem: their first motion phases are not certified and retry, and take their
    wave-mates' phases with them; the telemetry, phase by phase (prefix solves), is what the numpy restatement predicts"""
    B, K = 6, 5
    b = problems.make_batch("solo12_trot", B)
    Lx = np.where(np.arange(B) % 3 == 0, 1e4, 2.25e6)
    X0, F0, P0 = b.warm_start()

    def solve(k):
        return bb.solve_host(b, num_iters=k, warm=(X0, F0, P0), L_x=Lx, keep_hist=True, cert_phases=True)
    got = _switches(knobs, hiplib, lambda: solve(K))
    assert got[1]["stats"][:, 4].sum() > 0
    assert np.all(got[0]["cert_phases"] == 0) and np.all(got[2]["cert_phases"][:, 1] == 0)
    assert np.array_equal(got[2]["cert_phases"][:, 0], got[1]["cert_phases"][:, 0])
    pred = cr.phase_predictions(b, oracle, K, warm=(X0, F0, P0), L_x=Lx)
    knobs("bmpc_set_certified_steps", 1)
    counts = np.stack([np.zeros((B, 2), int)] + [solve(k)["cert_phases"] for k in range(1, K)] + [got[1]["cert_phases"]])      # [K + 1][B][2]
    ran = np.diff(counts, axis=0).transpose(1, 0, 2).astype(bool)                                                           # [B][K][2]
    for col, which in enumerate(("force", "motion")):
        want, usable = cr.wave_phases(pred, which)
        print(which, "predicted", want.astype(int).tolist(), "kernel", ran[:, :, col].astype(int).tolist(), "left out", int((pred["ran"] & ~usable).sum()))
        assert (pred["ran"] & ~usable).sum() * 10 <= pred["ran"].sum()
        assert np.array_equal(ran[:, :, col][usable], want[usable]), which
    assert not cr.wave_phases(pred, "motion")[0][:, 0][:4].any() and cr.wave_phases(pred, "motion")[0][:, 0][4:].all()


def test_floor_hand_over(hiplib, knobs):
    """tol far below machine precision: the motion FISTA runs until its steps vanish, |d|^2 falls under the certified loop's floor and
    the phase goes on in the tested loop -- with the bits and the iteration count of a phase tested throughout"""
    b = problems.make_batch("solo12_trot", 2)
    got = _switches(knobs, hiplib, lambda: bb.solve_host(b, num_iters=1, tol=1e-30, maxit=4000, keep_hist=True, cert_phases=True), values=(0, 1))
    assert np.array_equal(got[1]["cert_phases"], np.ones((2, 2), int))
    assert np.array_equal(got[0]["stats"][:, 2], got[1]["stats"][:, 2])
    print("motion FISTA iterations", got[1]["stats"][:, 2].tolist(), "force", got[1]["stats"][:, 1].tolist())


def test_divergence(hiplib, knobs):
    """Go2 at the reference's mu = 1 diverges (NaN) on some problems: alike under every value of the switch, and a diverged problem's
    wave-mate keeps the bits it has with the switch off"""
    b = problems.make_batch("go2_bound", 8, H=20)
    got = _switches(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, mu=1.0, keep_hist=True, cert_phases=True))
    bad = got[0]["stats"][:, 5] == 2
    assert bad.any()
    mates = [i ^ 1 for i in np.flatnonzero(bad) if not bad[i ^ 1]]
    print("diverged", np.flatnonzero(bad).tolist(), "wave-mates that did not", mates)
    for i in mates:
        for k in ("X", "F", "P"):
            assert np.all(np.isfinite(got[1][k][i])) and np.array_equal(got[1][k][i], got[0][k][i])
