"""Bipeds (n_eff = 2) without a GPU: the synthetic biped problem generator, its committed fixtures (tests/golden/make_golden_biped.py,
the biped_walk ensemble of tools/chaos_ensemble.py), the host side of a two-footed BiconvexMP handle against the C oracle, and the
batch descriptor's check of the foot count."""
import ctypes as C
import os

import numpy as np
import pytest

from bunmpc_amd import _lib, problems
from bunmpc_amd.biconvex_mpc_cpp import BiconvexMP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_biped_generator_is_deterministic_and_two_footed():
    b = problems.make_batch("biped_walk", 12)
    H = problems.BIPED_WALK.horizon
    assert (b.B, b.H, b.E) == (12, H, 2) and H == 20
    assert b.cnt_plan.shape == (12, H, 2, 4) and b.dt.shape == (12, H) and b.swing_time.shape == (12, H, 2)
    assert b.W_F.shape == (12, 6 * H) and b.W_X.shape == (12, 9 * H) and b.X_nom.shape == (12, 9 * H)
    assert b.m == problems.BIPED.mass and b.mu == problems.BIPED_MU
    X, F, P = b.warm_start()
    assert X.shape == (12, 9 * (H + 1)) and F.shape == (12, 3 * 2 * H)
    # per-problem draws: problem i is the same whatever the batch size or the first index
    again = problems.make_batch("biped_walk", 20)
    tail = problems.make_batch("biped_walk", 8, first=4)
    for k in ("cnt_plan", "dt", "x_init", "X_nom", "X_ter", "W_X", "W_X_ter", "W_F"):
        assert np.array_equal(getattr(again, k)[:12], getattr(b, k)), k
        assert np.array_equal(getattr(tail, k), getattr(b, k)[4:12]), k
    # both gaits drawn; a walk has double-support knots, a hop has flight knots (no foot on the ground)
    assert set(b.gait_id.tolist()) == {0, 1}
    flags = b.cnt_plan[..., 0]
    walk, hop = b.gait_id == 0, b.gait_id == 1
    assert np.any(flags[walk].sum(axis=2) == 2) and np.all(flags[walk].sum(axis=2) >= 1)
    assert np.any(flags[hop].sum(axis=2) == 0) and np.all(flags[hop][..., 0] == flags[hop][..., 1])


def test_contact_plan_takes_the_foot_count_from_the_gait():
    stand = problems.BIPED_STAND
    B, H = 3, 10
    feet0 = np.zeros((B, 2, 3))
    feet0[:, :, 0:2] = problems.BIPED.feet_xy
    feet0[:, :, 2] = problems.FOOT_SIZE
    cnt, swing, dt = problems.contact_plan(stand, problems.BIPED, H, np.zeros(B), np.zeros((B, 2)), np.full(B, 0.3), feet0,
                                           np.zeros((B, 3)), np.zeros(B))
    assert cnt.shape == (B, H, 2, 4) and swing.shape == (B, H, 2)
    assert np.all(cnt[..., 0] == 1) and np.all(cnt[:, :, :, 1:4] == feet0[:, None])     # standing still: the feet never move


def test_fixture_generator_reproduces_the_committed_file(oracle):
    from tests.golden import make_golden_biped as mg
    for name, config, B, iters in mg.CASES:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        f = mg.fixture(config, B, iters)
        assert sorted(g.files) == sorted(f)
        for k, v in f.items():
            assert np.array_equal(np.asarray(v), g[k]), k
        assert np.all(g["stats"][:, 5] == 0) and np.all(np.isfinite(g["X"])) and np.all(np.isfinite(g["F"]))


def test_committed_biped_chaos_ensemble_reproduces(oracle):
    """tests/golden/chaos_biped_walk.npz (tools/chaos_ensemble.py): its C members, re-run on every fourth sampled problem, give the
    committed k_calm / spreads / strict history exactly, as tests/test_oracle_cpu.py checks for the quadruped ensembles."""
    from tests.util import chaos_ensemble
    g = np.load(os.path.join(GOLDEN, "chaos_biped_walk.npz"))
    pick = np.arange(0, len(g["sub"]), 4)
    sub = g["sub"][pick]
    iters = int(g["iters"])
    b = problems.make_batch("biped_walk", 4096)
    ref, ens = chaos_ensemble(b.take(sub), sub, iters, oracle)
    assert np.array_equal(ref["trace"], g["ref_trace"][pick]) and np.array_equal(ref["hist"], g["ref_hist"][pick], equal_nan=True)
    assert np.array_equal(ens["k_calm"], g["k_calm_c"][pick])
    assert np.allclose(ens["spread"], g["spread_c"][pick], rtol=1e-9, atol=0)
    assert np.allclose(ens["hist_spread"], g["hist_spread_c"][pick], rtol=1e-9, atol=0)
    assert np.all(g["k_calm"] <= g["k_calm_c"]) and np.all(g["spread"] >= g["spread_c"])
    assert np.all(g["ref_stats"][:, 5] == 0)          # no sampled problem diverges


def _biped_handle(b, i):
    mp = BiconvexMP(b.m, b.H, 2)
    mp.set_rho(b.rho)
    for t in range(b.H):
        mp.set_contact_plan(b.cnt_plan[i, t], b.dt[i, t])
    return mp


def test_two_footed_handle_host_side_matches_oracle(oracle):
    """A BiconvexMP(m, H, 2) handle: A_x / b_x / A_f / b_f against the C oracle; the cost setters and the bound builder take the
    two-footed shapes (3 * 2 * H force entries) and refuse the four-footed ones.  (What they build reaches the solve: the drop-in test
    of tests/test_biped_gpu.py holds it to the oracle.)"""
    b = problems.make_batch("biped_walk", 3)
    i = 2
    mp = _biped_handle(b, i)
    assert mp.n_eff == 2 and mp.nf == 6 * b.H
    rng = np.random.default_rng(7)
    X = rng.standard_normal(9 * (b.H + 1))
    F = rng.standard_normal(6 * b.H)
    A, bx = oracle.dense_A_x(b.cnt_plan[i], b.dt[i], b.m, X)
    assert A.shape == (9 * (b.H + 1), 6 * b.H)
    assert np.array_equal(mp.return_A_x(X), A) and np.array_equal(mp.return_b_x(X), bx)
    A, bf = oracle.dense_A_f(b.cnt_plan[i], b.dt[i], b.m, F, b.x_init[i])
    assert np.allclose(mp.return_A_f(F, b.x_init[i]), A, rtol=0, atol=1e-15)
    assert np.allclose(mp.return_b_f(F, b.x_init[i]), bf, rtol=0, atol=1e-15)
    mp.create_bound_constraints(b.bounds[0], 15.0, 15.0, 15.0)
    mp.create_cost_X(b.W_X[i], b.W_X_ter[i], b.X_ter[i], b.X_nom[i])
    mp.create_cost_F(b.W_F[i])
    mp.set_cost_f(np.diag(b.W_F[i]), np.zeros(6 * b.H))
    mp.set_bounds_f(np.full(6 * b.H, -20.0), np.full(6 * b.H, 20.0))
    for bad in (lambda: mp.create_cost_F(np.ones(12 * b.H)), lambda: mp.set_bounds_f(np.zeros(12 * b.H), np.zeros(12 * b.H)),
                lambda: mp.set_contact_plan(np.zeros((4, 4)), 0.05)):
        with pytest.raises(ValueError):
            bad()
    # the contact plan is complete: the (H + 1)-th append is refused, as for four feet
    with pytest.raises(_lib.BmpcError):
        mp.set_contact_plan(b.cnt_plan[i, 0], 0.05)


def _host_descriptor(b, n_eff):
    d = _lib.Batch()
    _lib.lib().bmpc_batch_defaults(C.byref(d))
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (b.cnt_plan, b.dt, b.x_init, b.W_X, b.W_X_ter, b.W_F, b.bounds,
                                                                  b.X_nom, b.X_ter)]
    d.B, d.n_col, d.n_eff, d.raw, d.cold_start = b.B, b.H, n_eff, 0, 1
    d.m, d.rho = b.m, b.rho
    (d.cnt_plan, d.dt, d.x_init, d.W_X, d.W_X_ter, d.W_F, d.bounds, d.X_nom, d.X_ter) = [a.ctypes.data for a in keep]
    outs = [np.zeros(b.B * 9 * (b.H + 1)), np.zeros(b.B * 3 * n_eff * b.H), np.zeros(b.B * 9 * (b.H + 1)), np.zeros(b.B),
            np.zeros(b.B)]
    d.X, d.F, d.P, d.L_x, d.L_f = [a.ctypes.data for a in outs]
    return d, keep + outs


@pytest.mark.parametrize("n_eff", [1, 3, 5, 6])
def test_unsupported_foot_counts_are_refused_before_any_device_call(n_eff):
    """check_batch runs before anything touches a device: n_eff outside {2, 4} is BMPC_BAD_ARG with a message naming the supported
    set, on a machine without a GPU too."""
    b = problems.make_batch("biped_walk", 2)
    d, keep = _host_descriptor(b, n_eff)
    assert _lib.lib().bmpc_biconvex_solve_batch_host(C.byref(d)) == _lib.BAD_ARG
    msg = _lib.lib().bmpc_last_error().decode()
    assert "2" in msg and "4" in msg and "n_eff" in msg, msg
    assert _lib.lib().bmpc_biconvex_solve_batch_device(C.byref(d), None) == _lib.BAD_ARG
    del keep


def test_scratch_query_refuses_other_foot_counts(hiplib):
    for n_eff, precision in ((3, 0), (6, 1), (2, 2), (4, -1)):
        assert hiplib.bmpc_biconvex_kernel_scratch_bytes(n_eff, precision) == -1
        assert b"n_eff" in hiplib.bmpc_last_error()
