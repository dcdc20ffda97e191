"""The headline kernel's certified force loop with two feet per lane (bmpc_set_force_foot_pairs; DESIGN.md section 4, "Force loop: two feet
per lane"): mode 1 against mode 0 on the loop-constants build, by value (np.array_equal, NaN-aware) on X, F, P, stats, L_x, L_f, trace,
hist and dyn_viol -- with the helpers of tests/test_loop_constants_gpu.py.  bmpc_force_foot_pair_phases says how many (wave, force phase)
pairs took the new loop: it must be 0 in mode 0 and where the eligibility rule refuses, and what the case expects otherwise."""
import numpy as np
import pytest

from bunmpc_amd import problems
from tests.test_loop_constants_gpu import KEYS, _same, _solve, knobs  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu


def _modes(knobs, hiplib, solve):
    """solve() with two feet per lane and without: (the run with, its count of paired phases); every output equal, no paired phase without"""
    knobs("bmpc_set_force_foot_pairs", 1)
    hiplib.bmpc_force_foot_pair_phases(1)
    new = solve()
    n = hiplib.bmpc_force_foot_pair_phases(1)
    knobs("bmpc_set_force_foot_pairs", 0)
    old = solve()
    assert hiplib.bmpc_force_foot_pair_phases(1) == 0
    _same(new, old, "four feet per lane")
    return new, n


@pytest.mark.parametrize("H", [20, 16, 17])
def test_cold_starts(hiplib, knobs, H):
    """the benchmark's plan: 12 knots of two contacts, 8 of four at H = 20 -- 28 units; two waves (one with a padding segment), three
    certified force phases each"""
    b = problems.make_batch("solo12_trot", 3, H=H)
    got, n = _modes(knobs, hiplib, lambda: _solve(b, num_iters=3))
    assert np.all(got["stats"][:, 5] == 0) and np.array_equal(got["cert_phases"], np.full((3, 2), 3))
    assert n == 6


def test_mixed_gaits(hiplib, knobs):
    """two problems of every gait of solo12_mixed, each pair in a wave of its own: 26 .. 28 units"""
    m = problems.make_batch("solo12_mixed", 24, H=20)
    idx = [i for g in np.unique(m.gait_id) for i in np.flatnonzero(m.gait_id == g)[:2]]
    assert 4 <= len(idx) <= 6, (idx, m.gait_id.tolist())
    b = m.take(idx)
    got, n = _modes(knobs, hiplib, lambda: _solve(b, num_iters=3))
    print("gaits", m.gait_id[idx].tolist(), "paired phases", n, "certified", got["cert_phases"].tolist())
    assert n > 0


@pytest.mark.parametrize("maxit", [1, 2, 3, 4])
def test_loop_ends_by_the_iteration_cap(hiplib, knobs, maxit):
    b = problems.make_batch("solo12_trot", 3, H=20)
    got, n = _modes(knobs, hiplib, lambda: _solve(b, num_iters=3, maxit=maxit))
    assert np.all(got["stats"][:, 1] == 3 * maxit)
    assert n == 6


def test_wave_mates_leave_at_different_iterations(hiplib, knobs):
    b = problems.make_batch("solo12_trot", 3, H=20)
    got, n = _modes(knobs, hiplib, lambda: _solve(b, num_iters=3, tol=1e-3))
    print("FISTA iterations (force, motion)", got["stats"][:, 1:3].tolist(), "paired phases", n)
    assert got["stats"][0, 1] != got["stats"][1, 1]
    assert n > 0


def test_floor_hand_over_replays_the_phase(hiplib, knobs):
    """tol = 1e-30 (the case of tests/test_scalar_diet_gpu.py): a step falls below the floor, the new loop stores nothing and the phase
    runs again on four feet, which hands over to the tested loop"""
    b = problems.make_batch("solo12_trot", 3, H=20)
    got, n = _modes(knobs, hiplib, lambda: _solve(b, num_iters=3, tol=1e-30, maxit=4000))
    print("FISTA iterations per ADMM iteration (force)", got["trace"][:, :, 0].tolist(), "paired phases", n)


def test_knots_without_contact_and_with_three(hiplib, knobs):
    b = problems.make_batch("solo12_trot", 2, H=20)
    b.cnt_plan[:, 5, :, 0] = 0.0
    b.cnt_plan[:, 6, :, 0] = [1.0, 1.0, 1.0, 0.0]
    b.cnt_plan[1, 9, :, 0] = [0.0, 1.0, 1.0, 1.0]
    got, n = _modes(knobs, hiplib, lambda: _solve(b, num_iters=3))
    assert n > 0


def test_an_all_stance_wave_mate_falls_back(hiplib, knobs):
    """problem 0 in full stance: 40 units, so its wave runs four feet per lane -- no paired phase is counted"""
    b = problems.make_batch("solo12_trot", 2, H=20)
    b.cnt_plan[0, :, :, 0] = 1.0
    got, n = _modes(knobs, hiplib, lambda: _solve(b, num_iters=3))
    assert np.all(got["cert_phases"][:, 0] > 0)
    assert n == 0


def test_a_warm_start_with_swing_forces_falls_back(hiplib, knobs):
    b = problems.make_batch("solo12_trot", 2, H=20)
    c = _solve(b, num_iters=4)
    F = c["F"].reshape(2, 20, 4, 3).copy()
    F[:, :, :, 2] = np.where(b.cnt_plan[:, :, :, 0] == 0, 0.5, F[:, :, :, 2])
    F = F.reshape(2, -1)

    def first():
        return _solve(b, num_iters=1, maxit=1, warm=(c["X"], F, c["P"]), L_x=c["L_x"], L_f=c["L_f"])
    got, n = _modes(knobs, hiplib, first)
    assert n == 0
    got, n = _modes(knobs, hiplib, lambda: _solve(b, num_iters=3, warm=(c["X"], F, c["P"]), L_x=c["L_x"], L_f=c["L_f"]))
    print("warm start with swing forces: paired phases", n, "certified", got["cert_phases"].tolist())


def test_a_diverged_wave_mate_stays_contained(hiplib, knobs):
    clean = problems.make_batch("solo12_trot", 4, H=20)
    bad = problems.make_batch("solo12_trot", 4, H=20)
    bad.x_init[0, 3] = bad.x_init[3, 3] = 1e200
    ref, _ = _modes(knobs, hiplib, lambda: _solve(clean, num_iters=10))
    got, n = _modes(knobs, hiplib, lambda: _solve(bad, num_iters=10))
    assert got["stats"][:, 5].tolist() == [2, 0, 0, 2]
    for i in (1, 2):
        for k in KEYS:
            assert np.array_equal(got[k][i], ref[k][i]), (i, k)


def test_a_problem_that_diverges_inside_a_force_phase(hiplib, knobs, oracle):
    """the synthetic Go2 (15 kg, four feet, H = 20: the headline kernel's shape) at mu = 1: the projection blows up to NaN in the first
    force step, on the CPU oracle too; the NaN pattern of F is mode 0's"""
    b = problems.make_batch("go2_bound", 2, H=20)
    b.mu = 1.0
    ref = oracle.solve_batch(b, num_iters=2)
    assert np.isnan(ref["F"]).any(axis=1).all(), "the case must diverge on the oracle"
    got, n = _modes(knobs, hiplib, lambda: _solve(b, num_iters=2))
    assert np.array_equal(np.isnan(got["F"]), np.isnan(ref["F"]))
    print("paired phases", n, "status", got["stats"][:, 5].tolist())
