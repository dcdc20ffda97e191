"""The fp64 batch kernels' step certificate (bmpc_set_certified_steps): a force step whose Hessian bound is
below (L/2)(1 - eta) runs its FISTA loop without the backtracking test.  The test cannot fire there, so the switch must not show in
any output: every mapping and build, both forms, warm starts with persisted step constants, step constants small enough to make
backtracking happen (the certificate fails and the tested loop runs), diverging problems -- all bit for bit, NaN-aware."""
import numpy as np
import pytest

from bunmpc_amd import batch as bb
from bunmpc_amd import problems
from tests.util import knobs, launch_record  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu

KEYS = ("X", "F", "P", "L_x", "L_f", "stats", "trace", "hist", "dyn_viol")


def _both(knobs, hiplib, solve):
    out = {}
    for on in (0, 1):
        knobs("bmpc_set_certified_steps", on)
        out[on] = solve()
        out[on]["kernel"] = launch_record(hiplib)
    assert out[0]["kernel"] == out[1]["kernel"]
    for k in KEYS:
        if k in out[0]:
            assert np.array_equal(out[0][k], out[1][k], equal_nan=True), (out[0]["kernel"], k)
    return out[1]


@pytest.mark.parametrize("config,B,H,three,w2,lpp", [
    ("solo12_trot", 64, None, 0, 1, 32), ("solo12_trot", 64, None, 0, 0, 32),
    ("solo12_trot", 66, None, 1, 1, 21), ("solo12_trot", 66, None, 1, 0, 21),
    ("solo12_mixed", 37, 14, 2, 1, 16), ("solo12_mixed", 37, 14, 2, 0, 16),
    ("solo12_trot", 9, 40, 2, 1, 64), ("solo12_trot", 9, 40, 2, 0, 64),
    ("biped_walk", 64, None, 0, 1, 32), ("biped_walk", 66, None, 1, 0, 21)])
def test_batch_kernels_cold_and_warm(hiplib, knobs, config, B, H, three, w2, lpp):
    """every lanes-per-problem and build of the batch kernel, four feet and two; a cold start, then a warm start from its results
    with the step constants it left behind"""
    b = problems.make_batch(config, B, H=H)
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    knobs("bmpc_set_three_per_wave", three)
    knobs("bmpc_set_two_waves_per_simd", w2)
    cold = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, keep_hist=True))
    assert cold["kernel"] == ("biconvex_admm_kernel", lpp, 2 if w2 else 1)
    warm = (cold["X"], cold["F"], cold["P"])
    _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=4, warm=warm, L_x=cold["L_x"], L_f=cold["L_f"], keep_hist=True))


@pytest.mark.parametrize("w2", [0, 1])
@pytest.mark.parametrize("three", [0, 1])
def test_small_step_constants_force_backtracking(hiplib, knobs, oracle, w2, three):
    """L0 far below the Hessian's bound on some problems: those phases are not certified and retry; their wave-mates' are. Raw form
    with a linear force cost."""
    b = problems.make_batch("solo12_trot", 24)
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    knobs("bmpc_set_three_per_wave", three)
    knobs("bmpc_set_two_waves_per_simd", w2)
    pre = oracle.solve_batch(b, num_iters=0)
    raw = {k: pre[k] for k in ("Qx", "qx", "lbx", "ubx", "Qf")}
    raw["qf"] = np.random.default_rng(5).normal(0.0, 1e-3, pre["Qf"].shape)
    Lx = np.where(np.arange(b.B) % 3 == 0, 1e4, 2.25e6)
    Lf = np.where(np.arange(b.B) % 4 == 1, 10.0, 506.25)
    X0, F0, P0 = b.warm_start()
    got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=5, raw=raw, warm=(X0, F0, P0), L_x=Lx, L_f=Lf, keep_hist=True))
    assert got["stats"][:, 3].sum() > 0 and got["stats"][:, 4].sum() > 0
    got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=5, raw={k: raw[k] for k in ("Qx", "qx", "lbx", "ubx", "Qf")},
                                                     warm=(X0, F0, P0), L_x=Lx, L_f=Lf, keep_hist=True))


@pytest.mark.parametrize("H", [20, 40])
def test_go2_at_mu_1_diverges_alike(hiplib, knobs, H):
    """Go2 at the reference's mu = 1 diverges (NaN) on many problems; with and without the certificate alike"""
    b = problems.make_batch("go2_bound", 40, H=H)
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, mu=1.0, keep_hist=True))
    assert (got["stats"][:, 5] == 2).any()


@pytest.mark.parametrize("H,B", [(100, 3), (150, 2), (200, 2)])
@pytest.mark.parametrize("w2", [0, 1])
def test_workgroup_kernels(hiplib, knobs, H, B, w2):
    """64 .. 255 knots: one problem per workgroup of two to four waves (the certificate and the sums across the waves through LDS)"""
    b = problems.make_batch("solo12_trot", B, H=H)
    knobs("bmpc_set_two_waves_per_simd", w2)
    got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=3, keep_hist=True))
    assert got["kernel"][0] == "biconvex_admm_wg_kernel"


def test_work_stealing_kernel(hiplib, knobs):
    """the work-stealing kernel (num_iters >= 25, more problems than three per SIMD)"""
    b = problems.make_batch("solo12_trot", 3200)
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    knobs("bmpc_set_three_per_wave", 2)
    got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=30, keep_hist=True))
    assert got["kernel"][0] == "biconvex_admm_steal_kernel"
