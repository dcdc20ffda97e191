"""Bipeds (n_eff = 2) on the MI355X: every mapping of the centroidal solve with two feet per knot, against the strict C oracle
(tests/util.py::prefix_parity, the per-problem CPU ensembles) and against each other bit for bit; the committed fixture; the
BiconvexMP drop-in; the scratch guard; KinoDynMP still refusing anything but a quadruped.  Large batches are compared with the
oracle on sampled problems and with each other in full."""
import os

import numpy as np
import pytest

from bunmpc_amd import _lib
from bunmpc_amd import batch as bb
from bunmpc_amd import problems
from tests.util import TOL_FP64 as TOL, chaos_ensemble, cpu_spread, knobs, launch_record, prefix_parity, problem_args, rel_l2  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_MEDIAN, FP32_P95, FP32_MAX = 5e-6, 1e-5, 1e-2      # tests/test_parity_envelope_gpu.py


def _parity(oracle, b, sub, iters, got, members=16, ens=None):
    """problems `sub` of batch b (results `got` for the whole batch, with hist / trace) against the strict oracle under their CPU
    ensemble (the committed one when given)"""
    if ens is None:
        ref, ens = chaos_ensemble(b.take(sub), sub, iters, oracle, members=members)
    else:
        ref = oracle.solve_batch(b.take(sub), num_iters=iters, trace=True)
    ok, rep = prefix_parity({k: got[k][sub] for k in ("X", "F", "hist", "trace")}, ref, ens)
    assert np.all(ok), {int(sub[i]): w for i, w in rep["why"].items()}
    calm = ens["k_calm"] >= iters
    assert np.array_equal(got["stats"][sub][calm], ref["stats"][calm]) and np.all(got["stats"][sub][:, 5] == 0)
    return rep


@pytest.fixture(scope="module")
def walk4096():
    """biped_walk, B = 4096, H = 20, with the committed ensemble of its 64 sampled problems (tools/chaos_ensemble.py)"""
    g = np.load(os.path.join(GOLDEN, "chaos_biped_walk.npz"))
    return problems.make_batch("biped_walk", 4096), g["sub"], dict(k_calm=g["k_calm"], hist_spread=g["hist_spread"], spread=g["spread"])


def test_golden_fixture_without_the_oracle():
    g = np.load(os.path.join(GOLDEN, "biped_walk_b4_it10.npz"))
    b = problems.make_batch(str(g["config"]), g["X"].shape[0])
    assert b.E == 2 and np.array_equal(b.cnt_plan, g["cnt_plan"]) and np.array_equal(b.W_F, g["W_F"])
    got = bb.solve_host(b, num_iters=int(g["num_iters"]))
    assert np.array_equal(got["stats"], g["stats"])
    for k in ("X", "F", "P"):
        assert np.all(rel_l2(got[k], g[k]) < TOL), k
    assert np.array_equal(got["L_x"], g["L_x"]) and np.array_equal(got["L_f"], g["L_f"])


def test_latency_mapping_and_exact_step_decisions(oracle, hiplib, knobs, walk4096):
    """B <= 1024, H <= 20: one problem per wave, one foot per half-wave.  Against the oracle on the sampled problems; the fp32 shortcut
    of the step decisions against every decision taken in fp64: every output bit for bit, with step constants low enough to force
    retries in both FISTA loops."""
    b, sub, ens = walk4096
    small = b.slice(0, 1024)
    got = bb.solve_host(small, num_iters=10, keep_hist=True)
    assert launch_record(hiplib)[:2] == ("biconvex_latency_kernel", 0)
    pick = sub < 1024
    _parity(oracle, small, sub[pick], 10, got, ens={k: v[pick] for k, v in ens.items()})
    b64 = problems.make_batch("biped_walk", 64)
    Lx = np.where(np.arange(64) % 3 == 0, 1e4, 2.25e6)
    Lf = np.where(np.arange(64) % 4 == 0, 10.0, 506.25)
    X0, F0, P0 = b64.warm_start()
    out = {}
    for exact in (0, 1):
        knobs("bmpc_set_exact_step_decisions", exact)
        out[exact] = bb.solve_host(b64, num_iters=10, warm=(X0, F0, P0), L_x=Lx, L_f=Lf, keep_hist=True)
        assert launch_record(hiplib)[0] == "biconvex_latency_kernel"
    for k in ("X", "F", "P", "L_x", "L_f", "stats", "trace", "hist", "dyn_viol"):
        assert np.array_equal(out[0][k], out[1][k], equal_nan=True), k
    assert out[0]["stats"][:, 3].sum() > 0 and out[0]["stats"][:, 4].sum() > 0


def test_three_and_two_problems_per_wave_both_builds(oracle, hiplib, knobs, walk4096):
    """H = 20 at B = 4096 with the one-knot-per-lane kernel: 21-lane segments (three problems per wave) and 32-lane segments, each in
    its one-wave and its two-waves-per-SIMD build.  The builds of one segment size agree bit for bit; the segment sizes agree bit for
    bit in X / F / P on every problem whose discrete path they share (the segment sums add the same terms in another order); the
    sampled problems against the oracle."""
    b, sub, ens = walk4096
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    out = {}
    for lpp, three in ((21, 1), (32, 0)):
        knobs("bmpc_set_three_per_wave", three)
        for wpe in (1, 2):
            knobs("bmpc_set_two_waves_per_simd", 1 if wpe == 2 else 0)
            out[lpp, wpe] = bb.solve_host(b, num_iters=10, keep_hist=True)
            assert launch_record(hiplib) == ("biconvex_admm_kernel", lpp, wpe)
        for k in ("X", "F", "P", "L_x", "L_f", "stats", "trace", "hist", "dyn_viol"):
            assert np.array_equal(out[lpp, 1][k], out[lpp, 2][k], equal_nan=True), (lpp, k)
        _parity(oracle, b, sub, 10, out[lpp, 1], ens=ens)
    a, c = out[21, 1], out[32, 1]
    same = np.all(a["trace"] == c["trace"], axis=(1, 2))
    assert same.mean() >= 0.9, same.mean()
    for k in ("X", "F", "P", "L_x", "L_f", "stats"):
        assert np.array_equal(a[k][same], c[k][same]), k
    for k in ("hist", "dyn_viol"):
        assert np.allclose(a[k][same], c[k][same], rtol=1e-12, atol=0, equal_nan=True), k


@pytest.mark.parametrize("H,lpp", [(15, 16), (40, 64)])
def test_sixteen_and_sixty_four_lanes_both_builds(oracle, hiplib, knobs, H, lpp):
    b = problems.make_batch("biped_walk", 96, H=H)
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    out = {}
    for wpe in (1, 2):
        knobs("bmpc_set_two_waves_per_simd", 1 if wpe == 2 else 0)
        out[wpe] = bb.solve_host(b, num_iters=10, keep_hist=True)
        assert launch_record(hiplib) == ("biconvex_admm_kernel", lpp, wpe)
    for k in ("X", "F", "P", "L_x", "L_f", "stats", "trace", "hist", "dyn_viol"):
        assert np.array_equal(out[1][k], out[2][k], equal_nan=True), k
    _parity(oracle, b, np.arange(0, 96, 8), 10, out[1])


def test_raw_form_on_the_batch_kernel(oracle, hiplib, knobs):
    """the raw cost / bound arrays (what a BiconvexMP handle's setters leave behind), with and without a linear force cost"""
    b = problems.make_batch("biped_walk", 12, H=20)
    ref = oracle.solve_batch(b, num_iters=0)
    raw = {k: ref[k] for k in ("Qx", "qx", "lbx", "ubx", "Qf")}
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    for qf in (None, 0.1 * np.ones_like(ref["Qf"])):
        got = bb.solve_host(b, num_iters=5, raw=dict(raw, qf=qf))
        assert launch_record(hiplib)[0] == "biconvex_admm_kernel"
        for i in range(b.B):
            r = oracle.biconvex_solve(*problem_args(b, i, raw), rho=b.rho, num_iters=5, mu=b.mu, qf=None if qf is None else qf[i])
            assert np.array_equal(got["stats"][i], r["stats"]), i
            for k in "XFP":
                assert rel_l2(got[k][i], r[k]) < TOL, (i, k)


def test_fp32_harness_form(oracle, hiplib):
    B = 256
    b = problems.make_batch("biped_walk", B)
    ref, spread = cpu_spread(b, 10, oracle, with_numpy=False)
    got = bb.solve_host(b, num_iters=10, precision="f32")
    assert launch_record(hiplib)[:2] == ("biconvex_admm_kernel_f32", 32)
    assert np.array_equal(got["stats"][:, [0, 5]], ref["stats"][:, [0, 5]])
    err = np.maximum(rel_l2(got["X"], ref["X"]), rel_l2(got["F"], ref["F"]))
    calm = spread <= 1e-9
    print("biped_walk fp32 vs CPU oracle: calm %d problems median %.2e p95 %.2e max %.2e" % (calm.sum(), np.median(err[calm]),
                                                                                       np.quantile(err[calm], 0.95), err[calm].max()))
    assert calm.mean() > 0.9
    assert np.median(err[calm]) <= FP32_MEDIAN and np.quantile(err[calm], 0.95) <= FP32_P95 and np.all(err[calm] <= FP32_MAX)
    F = got["F"].reshape(B, b.H, 2, 3)
    assert np.all(F[b.cnt_plan[..., 0] == 0] == 0.0) and np.all(F[..., 2] >= 0)


@pytest.mark.parametrize("H,lpp", [(100, 128), (160, 192), (200, 256)])
def test_one_problem_per_workgroup(oracle, hiplib, knobs, H, lpp):
    b = problems.make_batch("biped_walk", 3, H=H)
    out = {}
    for wpe in (1, 2):
        knobs("bmpc_set_two_waves_per_simd", 1 if wpe == 2 else 0)
        out[wpe] = bb.solve_host(b, num_iters=3, keep_hist=True)
        assert launch_record(hiplib) == ("biconvex_admm_wg_kernel", lpp, wpe)
    for k in ("X", "F", "P", "L_x", "L_f", "stats", "trace", "hist", "dyn_viol"):
        assert np.array_equal(out[1][k], out[2][k], equal_nan=True), k
    _parity(oracle, b, np.arange(3), 3, out[1], members=4)


def test_work_stealing_hundred_iterations(oracle, hiplib, knobs):
    """num_iters = 100 at B = 4096: the work-stealing kernel; everything as from the plain three-per-wave launch (X / F / P / counts bit
    for bit, the segment sums to 1e-12: they depend on which segment of a wave holds the problem), sampled problems against the oracle"""
    from bunmpc_amd import batch as bbm
    b = problems.make_batch("biped_walk", 4096)
    out = {}
    for on in (1, 0):
        knobs("bmpc_set_work_stealing", on)
        dev = bbm.DeviceBatch(b, num_iters=100, keep_hist=True)
        dev.solve()
        out[on] = dev.results()
        assert launch_record(hiplib)[:2] == ("biconvex_admm_steal_kernel" if on else "biconvex_admm_kernel", 21)
    n = out[1]["stats"][:, 0]
    print("biped work stealing: ADMM iterations min %d median %d max %d" % (n.min(), np.median(n), n.max()))
    for k in ("X", "F", "P", "L_x", "L_f", "stats", "trace"):
        assert np.array_equal(out[1][k], out[0][k]), k
    assert np.allclose(out[1]["dyn_viol"], out[0]["dyn_viol"], rtol=1e-12, atol=0)
    assert np.allclose(out[1]["hist"], out[0]["hist"], rtol=1e-12, atol=0, equal_nan=True)
    _parity(oracle, b, np.arange(0, 4096, 512), 100, out[1])


def _drive(mp, b, i, iters, warm=True):
    for t in range(b.H):
        mp.set_contact_plan(b.cnt_plan[i, t], b.dt[i, t])
    mp.create_bound_constraints(b.bounds[0], 15.0, 15.0, 15.0)
    mp.create_cost_X(b.W_X[i], b.W_X_ter[i], b.X_ter[i], b.X_nom[i])
    mp.create_cost_F(b.W_F[i])
    if warm:
        X0, F0, P0 = b.warm_start()
        mp.set_warm_start_vars(X0[i], F0[i], P0[i])
    mp.optimize(b.x_init[i], iters)


def test_dropin_biped_handle(oracle):
    """BiconvexMP(m, H, 2) driven as the reference's harness drives its planner: contact plan rows of shape (2, 4), optimize(x, 10);
    then a second optimize of the same handle with the step constants it carried over (fista.hpp:52)"""
    from bunmpc_amd.biconvex_mpc_cpp import BiconvexMP
    b = problems.make_batch("biped_walk", 3)
    ref = oracle.solve_batch(b, num_iters=10)
    for i in range(b.B):
        mp = BiconvexMP(b.m, b.H, 2)
        mp.set_rho(b.rho)
        mp.set_friction_coefficient(b.mu)
        _drive(mp, b, i, 10)
        assert rel_l2(mp.return_opt_x(), ref["X"][i]) < TOL
        assert rel_l2(mp.return_opt_f(), ref["F"][i]) < TOL
        assert rel_l2(mp.return_opt_p(), ref["P"][i]) < TOL
        assert np.array_equal(mp.last_stats(), ref["stats"][i])
        assert mp.return_opt_com().shape == (b.H + 1, 3)
    mp = BiconvexMP(b.m, b.H, 2)
    mp.set_rho(b.rho)
    mp.set_friction_coefficient(b.mu)
    mp.set_step_constants(2e5, 40.0)          # low enough to force retries that must persist
    _drive(mp, b, 0, 3)
    L1 = mp.step_constants()
    _drive(mp, b, 0, 3, warm=False)            # continues from the previous X / F / P and L
    pre = oracle.solve_batch(b.take([0]), num_iters=0)
    args = problem_args(b, 0, pre)
    r1 = oracle.biconvex_solve(*args, L_x=2e5, L_f=40.0, rho=b.rho, num_iters=3, mu=b.mu)
    assert (r1["L_x"], r1["L_f"]) == L1 and r1["stats"][3] > 0 and r1["stats"][4] > 0
    r2 = oracle.biconvex_solve(*args[:9], r1["X"], r1["F"], r1["P"], L_x=r1["L_x"], L_f=r1["L_f"], rho=b.rho, num_iters=3, mu=b.mu)
    assert rel_l2(mp.return_opt_x(), r2["X"]) < TOL and rel_l2(mp.return_opt_f(), r2["F"]) < TOL
    assert mp.step_constants() == (r2["L_x"], r2["L_f"])


def test_scratch_guard(hiplib):
    assert hiplib.bmpc_biconvex_kernel_scratch_bytes(2, 1) == 0
    assert hiplib.bmpc_biconvex_kernel_scratch_bytes(4, 1) == hiplib.bmpc_biconvex_fp32_scratch_bytes() == 0
    s2, s4 = hiplib.bmpc_biconvex_kernel_scratch_bytes(2, 0), hiplib.bmpc_biconvex_kernel_scratch_bytes(4, 0)
    print("fp64 batch kernels, largest scratch bytes per lane: two feet %d, four feet %d" % (s2, s4))
    assert 0 <= s2 <= s4


def test_kinodyn_still_refuses_two_feet():
    """the whole-body model is a 12-joint quadruped: KinoDynMP with n_eff = 2 is refused before any solve"""
    from bunmpc_amd import urdf_model
    from bunmpc_amd.biconvex_mpc_cpp import KinoDynMP
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model = urdf_model.RobotModel.from_json(open(os.path.join(root, "bunmpc_amd", "robots", "solo12.json")).read())
    with pytest.raises(_lib.BmpcError) as e:
        KinoDynMP(model, model.total_mass, 2, 20, 10)
    assert e.value.code == _lib.BAD_ARG and b"n_eff" in _lib.lib().bmpc_last_error()
