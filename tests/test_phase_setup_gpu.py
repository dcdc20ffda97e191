"""The headline kernel's phase set-up that is made once per solve ("Force loop: two feet per lane"): the unit map of
the force loop is built in front of the ADMM loop, from the contact plan, and every force phase reads its entry back.  Nothing may show in
any output: the default path against four feet per lane (bmpc_set_force_foot_pairs 0) and against the two-waves build without the loop
constants in LDS, by value (np.array_equal, NaN-aware) on X, F, P, stats, L_x, L_f, trace, hist and dyn_viol, with the helpers of
tests/test_loop_constants_gpu.py.  bmpc_force_foot_pair_phases counts the (wave, force phase) pairs that ran two feet per lane: 0 on both
other paths, and on the default path one per certified force phase of every wave whose plans fit -- a phase that finds a stale or
clobbered map either fails the comparison or is not counted."""
import numpy as np
import pytest

from bunmpc_amd import problems
from tests.test_loop_constants_gpu import KEYS, _same, _solve, knobs  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu


def _paths(knobs, hiplib, solve):
    """solve() on the default path (the returned run and its count of paired phases), with four feet per lane and on the two-waves build"""
    knobs("bmpc_set_loop_constants_in_lds", 1)
    knobs("bmpc_set_force_foot_pairs", 1)
    hiplib.bmpc_force_foot_pair_phases(1)
    new = solve()
    n = hiplib.bmpc_force_foot_pair_phases(1)
    knobs("bmpc_set_force_foot_pairs", 0)
    four = solve()
    assert hiplib.bmpc_force_foot_pair_phases(1) == 0
    _same(new, four, "four feet per lane")
    knobs("bmpc_set_force_foot_pairs", 1)
    knobs("bmpc_set_loop_constants_in_lds", 0)
    two = solve()
    assert hiplib.bmpc_force_foot_pair_phases(1) == 0
    _same(new, two, "the two-waves build")
    knobs("bmpc_set_loop_constants_in_lds", 1)
    return new, n


@pytest.mark.parametrize("H", [20, 16, 17])
def test_cold_starts(hiplib, knobs, H):
    """two waves, three certified force phases each: the second and third read a map they did not build"""
    b = problems.make_batch("solo12_trot", 3, H=H)
    got, n = _paths(knobs, hiplib, lambda: _solve(b, num_iters=3))
    assert np.all(got["stats"][:, 5] == 0) and np.array_equal(got["cert_phases"], np.full((3, 2), 3))
    assert n == 6


def test_ten_iterations_and_a_diverged_wave_mate_on_either_side(hiplib, knobs):
    """the benchmark's ten ADMM iterations; then problems 0 and 3 start at a velocity of 1e200 and are NaN after two iterations: problem 1
    sits behind a diverged problem, problem 2 in front of one, and both return the bits of the clean batch -- no NaN reaches them through
    the map or the phase's test of it"""
    clean = problems.make_batch("solo12_trot", 4, H=20)
    bad = problems.make_batch("solo12_trot", 4, H=20)
    bad.x_init[0, 3] = bad.x_init[3, 3] = 1e200
    ref, n = _paths(knobs, hiplib, lambda: _solve(clean, num_iters=10))
    print("ten iterations: paired phases", n, "certified (force, motion)", ref["cert_phases"].tolist())
    assert np.all(ref["stats"][:, 0] == 10)
    assert n == ref["cert_phases"][0, 0] + ref["cert_phases"][2, 0]      # (a certificate is the wave's: problems 0 and 2 speak for theirs)
    assert n > 6
    got, nb = _paths(knobs, hiplib, lambda: _solve(bad, num_iters=10))
    print("diverged wave-mates: paired phases", nb)
    assert got["stats"][:, 5].tolist() == [2, 0, 0, 2]
    for i in (1, 2):
        for k in KEYS:
            assert np.all(np.isfinite(got[k][i])), (i, k)
            assert np.array_equal(got[k][i], ref[k][i]), (i, k)


def test_the_map_survives_replayed_phases(hiplib, knobs):
    """tol = 1e-30: in every force phase a step falls below the floor, the paired loop stores nothing and the phase runs again on four
    feet, which hands over to the tested loop; the next phase pairs again from the same map"""
    b = problems.make_batch("solo12_trot", 3, H=20)
    got, n = _paths(knobs, hiplib, lambda: _solve(b, num_iters=2, tol=1e-30, maxit=4000))
    per_phase = np.diff(got["trace"][:, :, 0], axis=1, prepend=0)
    print("FISTA iterations per force phase", per_phase.tolist(), "paired phases", n)
    assert n == 0      # (a phase that replays is not counted, and none gets to the cap before its step is below the floor)


def test_the_map_survives_a_phase_on_four_feet(hiplib, knobs):
    """a warm start whose swing feet carry forces: the first force phase is not eligible and runs four feet per lane; whatever pairs
    later reads the map made before it"""
    b = problems.make_batch("solo12_trot", 2, H=20)
    c = _solve(b, num_iters=4)
    F = c["F"].reshape(2, 20, 4, 3).copy()
    F[:, :, :, 2] = np.where(b.cnt_plan[:, :, :, 0] == 0, 0.5, F[:, :, :, 2])
    F = F.reshape(2, -1)
    warm = dict(warm=(c["X"], F, c["P"]), L_x=c["L_x"], L_f=c["L_f"])
    got, n = _paths(knobs, hiplib, lambda: _solve(b, num_iters=1, maxit=1, **warm))
    assert n == 0
    got, n = _paths(knobs, hiplib, lambda: _solve(b, num_iters=3, **warm))
    print("warm start with swing forces: paired phases", n, "certified", got["cert_phases"].tolist())
    assert n == got["cert_phases"][0, 0] - 1      # (the first phase on four feet, the later ones paired)


def test_independent_segments(hiplib, knobs):
    """wave 0: two different gaits of solo12_mixed, two different maps in one wave; wave 1: a full-stance plan (40 units) beside a
    trot -- `fits` is the wave's, its map is not used"""
    m = problems.make_batch("solo12_mixed", 24, H=20)
    gaits = np.unique(m.gait_id)
    assert len(gaits) >= 2, m.gait_id.tolist()
    idx = [int(np.flatnonzero(m.gait_id == g)[0]) for g in gaits[:2]]
    t = int(np.flatnonzero(m.gait_id == gaits[0])[1])
    b = m.take(idx + [t, t])
    b.cnt_plan[2, :, :, 0] = 1.0
    got, n = _paths(knobs, hiplib, lambda: _solve(b, num_iters=3))
    print("gaits", m.gait_id[idx].tolist(), "paired phases", n, "certified", got["cert_phases"].tolist())
    assert got["cert_phases"][0, 0] > 0 and got["cert_phases"][2, 0] > 0
    assert n == got["cert_phases"][0, 0]


def test_knots_without_contact_and_with_three(hiplib, knobs):
    """a knot of no contact (one unit without slots) and knots of three (a second unit: every later knot's first unit moves up a lane),
    differently in the wave's two problems"""
    b = problems.make_batch("solo12_trot", 2, H=20)
    b.cnt_plan[:, 5, :, 0] = 0.0
    b.cnt_plan[:, 6, :, 0] = [1.0, 1.0, 1.0, 0.0]
    b.cnt_plan[1, 9, :, 0] = [0.0, 1.0, 1.0, 1.0]
    got, n = _paths(knobs, hiplib, lambda: _solve(b, num_iters=3))
    assert got["cert_phases"][0, 0] > 0
    assert n == got["cert_phases"][0, 0]


@pytest.mark.parametrize("maxit", [1, 2])
def test_iteration_caps(hiplib, knobs, maxit):
    b = problems.make_batch("solo12_trot", 3, H=20)
    got, n = _paths(knobs, hiplib, lambda: _solve(b, num_iters=3, maxit=maxit))
    assert np.all(got["stats"][:, 1] == 3 * maxit)
    assert n == 6


@pytest.mark.parametrize("tol", [1e-3, 3e-4])
def test_exits_with_the_quad_stage_of_the_screen(hiplib, knobs, oracle, tol):
    """problems 0, 1, 3, 7 of the perturbed batch at tolerances at which they leave their phases below the cap, at different iterations:
    the stage between the lane's partial and the segment sum (biconvex_lanes.h: quad_screen; tests/test_quad_screen_cpu.py) settles
    iterations near every one of these exits and may move none of them -- the FISTA counts per ADMM iteration (trace) are those of
    the two-waves build, which has no such stage, and of the CPU oracle"""
    b = problems.make_batch("solo12_trot", 8, H=20).take([0, 1, 3, 7])
    ref = oracle.solve_batch(b, num_iters=3, tol=tol, trace=True)["trace"]
    got, n = _paths(knobs, hiplib, lambda: _solve(b, num_iters=3, tol=tol))
    print("tol", tol, "FISTA iterations (force, motion)", got["stats"][:, 1:3].tolist(), "oracle", ref[:, -1, :2].tolist(), "paired phases", n)
    assert np.all(got["stats"][:, 1:3] < 3 * 150), "every problem leaves some phase below the cap"
    assert np.array_equal(got["trace"][:, :, :2], ref[:, :, :2])
    assert n > 0
