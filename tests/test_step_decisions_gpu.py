"""The fp32 step decisions of the batch kernel (biconvex_admm_body.h: BAND): a decision is taken from the fp32
segment sums only where it is the one the fp64 sums make, so bmpc_set_exact_step_decisions must not show in any output.  The shortcut
is compiled into ONE instantiation, the two-waves-per-SIMD build at 32 lanes, four feet, harness form (the benchmark's kernel):
test_headline_dispatch and test_shortcut_kernel_* exercise it -- cold and warm starts, retries in both loops, a diverging problem,
a negative weight (the shortcut off for the wave).  The other cases run kernels without it and only guard that the switch does not
reach them.  All bit for bit, NaN-aware."""
import numpy as np
import pytest

from bunmpc_amd import batch as bb
from bunmpc_amd import problems
from tests.util import knobs, launch_record  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu

KEYS = ("X", "F", "P", "L_x", "L_f", "stats", "trace", "hist", "dyn_viol")


def _both(knobs, hiplib, solve, keys=KEYS):
    out = {}
    for exact in (0, 1):
        knobs("bmpc_set_exact_step_decisions", exact)
        out[exact] = solve()
        out[exact]["kernel"] = launch_record(hiplib)
    assert out[0]["kernel"] == out[1]["kernel"]
    for k in keys:
        if k in out[0]:
            assert np.array_equal(out[0][k], out[1][k], equal_nan=True), (out[0]["kernel"], k)
    return out[1]


def test_headline_dispatch(hiplib, knobs):
    """the benchmark's launch: B = 4096 Solo12 trot, H = 20, the default dispatch"""
    b = problems.make_batch("solo12_trot", 4096)
    got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, keep_hist=True))
    assert got["kernel"] == ("biconvex_admm_kernel", 32, 2)


@pytest.mark.parametrize("case", ["cold_warm", "retries", "diverging", "negative_weight"])
def test_shortcut_kernel(hiplib, knobs, case):
    """the kernel with the shortcut, at a small batch"""
    b = problems.make_batch("solo12_trot", 256)
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    knobs("bmpc_set_three_per_wave", 0)
    knobs("bmpc_set_two_waves_per_simd", 1)
    X0, F0, P0 = b.warm_start()
    if case == "cold_warm":
        got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, keep_hist=True))
        warm = (got["X"], got["F"], got["P"])
        _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=4, warm=warm, L_x=got["L_x"], L_f=got["L_f"], keep_hist=True))
    elif case == "retries":
        Lx = np.where(np.arange(b.B) % 3 == 0, 1e4, 2.25e6)
        Lf = np.where(np.arange(b.B) % 4 == 1, 10.0, 506.25)
        got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, warm=(X0, F0, P0), L_x=Lx, L_f=Lf, keep_hist=True))
        assert got["stats"][:, 3].sum() > 0 and got["stats"][:, 4].sum() > 0
    elif case == "diverging":
        b.x_init[5, 2] = 1e200
        b.X_nom[5] = 1e200
        got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, keep_hist=True))
        assert got["stats"][5, 5] == 2
    else:
        b.W_X = np.array(b.W_X, copy=True)
        b.W_X.reshape(-1)[4] = -1e-3
        got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, keep_hist=True))
    assert got["kernel"] == ("biconvex_admm_kernel", 32, 2)


@pytest.mark.parametrize("config,B,H,three,w2,lpp", [
    ("solo12_trot", 512, None, 0, 0, 32),
    ("solo12_trot", 66, None, 1, 1, 21), ("solo12_trot", 66, None, 1, 0, 21),
    ("solo12_mixed", 37, 14, 2, 1, 16), ("solo12_mixed", 37, 14, 2, 0, 16),
    ("solo12_trot", 9, 40, 2, 1, 64), ("solo12_trot", 9, 40, 2, 0, 64),
    ("biped_walk", 64, None, 0, 1, 32), ("biped_walk", 66, None, 1, 0, 21)])
def test_batch_kernels_cold_and_warm(hiplib, knobs, config, B, H, three, w2, lpp):
    """every lanes-per-problem and build of the batch kernel, four feet and two; a cold start, then a warm start from its results"""
    b = problems.make_batch(config, B, H=H)
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    knobs("bmpc_set_three_per_wave", three)
    knobs("bmpc_set_two_waves_per_simd", w2)
    cold = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, keep_hist=True))
    assert cold["kernel"] == ("biconvex_admm_kernel", lpp, 2 if w2 else 1)
    warm = (cold["X"], cold["F"], cold["P"])
    _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=4, warm=warm, L_x=cold["L_x"], L_f=cold["L_f"], keep_hist=True))


@pytest.mark.parametrize("three", [0, 1])
def test_raw_form_retries_and_a_negative_weight(hiplib, knobs, oracle, three):
    """raw form with a linear force cost and step constants low enough to make both loops retry; then a negative state weight in
    one problem (its wave takes every motion decision from the fp64 sums)"""
    b = problems.make_batch("solo12_trot", 24)
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    knobs("bmpc_set_three_per_wave", three)
    pre = oracle.solve_batch(b, num_iters=0)
    raw = {k: pre[k] for k in ("Qx", "qx", "lbx", "ubx", "Qf")}
    raw["qf"] = np.random.default_rng(5).normal(0.0, 1e-3, pre["Qf"].shape)
    Lx = np.where(np.arange(b.B) % 3 == 0, 1e4, 2.25e6)
    Lf = np.where(np.arange(b.B) % 4 == 1, 10.0, 506.25)
    X0, F0, P0 = b.warm_start()
    got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=5, raw=raw, warm=(X0, F0, P0), L_x=Lx, L_f=Lf, keep_hist=True))
    assert got["stats"][:, 3].sum() > 0 and got["stats"][:, 4].sum() > 0
    neg = dict(raw)
    neg["Qx"] = raw["Qx"].copy()
    neg["Qx"][1, 9 * 3 + 4] = -1e-3
    _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=5, raw=neg, warm=(X0, F0, P0), L_x=Lx, L_f=Lf, keep_hist=True))


def test_go2_bound_retries_and_divergence(hiplib, knobs):
    """Go2 bound (H = 40: 64 lanes): its force phases are not all certified, so the tested loop runs; step constants low enough to make
    both loops retry; at the reference's mu = 1 many problems diverge (inf / NaN sums)"""
    b = problems.make_batch("go2_bound", 40)
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, keep_hist=True))
    X0, F0, P0 = b.warm_start()
    Lx = np.where(np.arange(b.B) % 3 == 0, 1e4, 2.25e6)
    Lf = np.where(np.arange(b.B) % 4 == 1, 10.0, 506.25)
    got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, warm=(X0, F0, P0), L_x=Lx, L_f=Lf, keep_hist=True))
    assert got["stats"][:, 3].sum() > 0 and got["stats"][:, 4].sum() > 0
    got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=10, mu=1.0, keep_hist=True))
    assert (got["stats"][:, 5] == 2).any()


def test_work_stealing_kernel_at_100_iterations(hiplib, knobs):
    """the work-stealing kernel at the reference's num_iters = 100.  The iterates, counts and per-iteration path (`trace`) must agree;
    the violation norms (`hist`, `dyn_viol`) are left out: a stolen problem runs in whichever 21-lane segment is free, and the sum
    of its violation adds the lanes in that segment's order, so those differ in the last bit from one run to the next with the same
    setting, the parent's kernel alike"""
    b = problems.make_batch("solo12_trot", 3200)
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    got = _both(knobs, hiplib, lambda: bb.solve_host(b, num_iters=100, keep_hist=True), keys=("X", "F", "P", "L_x", "L_f", "stats", "trace"))
    assert got["kernel"][0] == "biconvex_admm_steal_kernel"
