"""The certified loops of the loop-constants build after their scalar diet ("Certified loops: scalar diet"): iteration
counts from the exit index, the last iteration's store at the loop's exit, `act` and the screen's words changed only where a problem
finishes, a scalar momentum coefficient, the constants waited for once per batch, idle lanes on LDS banks of their own.  None of it may
show in any output: every case compares bmpc_set_loop_constants_in_lds 1 against 0 (the two-waves build, which keeps the shared loops)
and against the one-wave build, bit for bit, on X, F, P, stats, L_x, L_f, trace, hist and dyn_viol -- with the helpers of
tests/test_loop_constants_gpu.py, as that file compares.  B = 3 unless a case needs named problems: a full wave and a half-empty one."""
import numpy as np
import pytest

from bunmpc_amd import problems
from tests.test_loop_constants_gpu import KEYS, _builds, _solve, knobs  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H", [20, 16, 17])
def test_cold_starts(hiplib, knobs, H):
    """H + 1 = 21 (the benchmark's), 17 (the shortest segment of 32 lanes) and 18 (the other horizon at which the parent's layout had
    every idle lane on a knot lane's bank)"""
    b = problems.make_batch("solo12_trot", 3, H=H)
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3))
    assert np.all(got["stats"][:, 0] == 3) and np.all(got["stats"][:, 5] == 0)
    assert np.array_equal(got["cert_phases"], np.full((3, 2), 3))


def test_warm_start(hiplib, knobs):
    b = problems.make_batch("solo12_trot", 3, H=20)
    c = _solve(b, num_iters=10)
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=4, warm=(c["X"], c["F"], c["P"]), L_x=c["L_x"], L_f=c["L_f"]))
    print("warm start: certified phases", got["cert_phases"].tolist(), "FISTA iterations", got["stats"][:, 1:3].tolist())


@pytest.mark.parametrize("maxit", [1, 2, 3, 4])
def test_loop_ends_by_the_iteration_cap(hiplib, knobs, maxit):
    """every phase ends at iteration maxit - 1: the store at the loop's exit from the register set that iteration wrote -- xb / rb behind
    an even index (maxit 1, 3), xa / ra behind an odd one (2, 4) -- and the exit tests of the first and the second copy"""
    b = problems.make_batch("solo12_trot", 3, H=20)
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3, maxit=maxit))
    assert np.all(got["stats"][:, 1] == 3 * maxit) and np.all(got["stats"][:, 2] == 3 * maxit)
    assert np.array_equal(got["cert_phases"], np.full((3, 2), 3))


def test_wave_mates_leave_at_different_iterations(hiplib, knobs, oracle):
    """tol = 1e-3, problems 0 and 1 of the perturbed batch in one wave: their counts differ in both phases (CPU oracle: 215 / 99 and
    204 / 104 after three ADMM iterations), so each phase has a problem whose count is the index at which its bit fell while its mate
    goes on with the screen's word of that half set"""
    b = problems.make_batch("solo12_trot", 3, H=20)
    ref = oracle.solve_batch(b, num_iters=3, tol=1e-3, trace=True)["trace"]
    assert ref[0, -1, 0] != ref[1, -1, 0] and ref[0, -1, 1] != ref[1, -1, 1], ref[:2, -1].tolist()
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3, tol=1e-3))
    print("FISTA iterations (force, motion)", got["stats"][:, 1:3].tolist(), "oracle", ref[:, -1, :2].tolist())
    assert got["stats"][0, 1] != got["stats"][1, 1] and got["stats"][0, 2] != got["stats"][1, 2]
    assert np.all(got["cert_phases"] > 0)


def test_wave_mates_leave_in_the_same_iteration(hiplib, knobs, oracle):
    """a tolerance and two problems, picked on the CPU oracle, that finish a phase of the first ADMM iteration in the same FISTA
    iteration below the cap: both bits fall at once and the loop ends with nobody left"""
    eight = problems.make_batch("solo12_trot", 8, H=20)
    pick = None
    for tol in (3e-4, 1e-3, 3e-3, 1e-2):
        ref = oracle.solve_batch(eight, num_iters=1, tol=tol, trace=True)["trace"][:, 0, :2]
        pick = next(((tol, i, j, ph) for ph in (0, 1) for i in range(8) for j in range(i + 1, 8) if ref[i, ph] == ref[j, ph] < 150), None)
        if pick:
            break
    assert pick, "no pair on the oracle"
    tol, i, j, ph = pick
    b = eight.take([i, j])
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=1, tol=tol))
    print("tol", tol, "problems", (i, j), "phase", ph, "FISTA iterations (force, motion)", got["stats"][:, 1:3].tolist())
    assert got["stats"][0, 1 + ph] == got["stats"][1, 1 + ph] < 150
    assert np.all(got["cert_phases"][:, ph] == 1)


def test_a_problem_leaves_at_exactly_the_last_iteration(hiplib, knobs, oracle):
    """maxit set to the smaller of the two iteration counts that problems 0 and 1 have in their first force phase at tol = 1e-3 (CPU
    oracle: 90 and 88; the first phase of a cold start does not depend on maxit up to the cap): that problem's `done` bit rises at index
    maxit - 1 -- latched there, not stored at the exit -- while its wave-mate is still iterating when the loop ends and is stored at
    the exit"""
    b = problems.make_batch("solo12_trot", 3, H=20)
    ref = oracle.solve_batch(b, num_iters=1, tol=1e-3, trace=True)["trace"][:, 0, 0]
    n = int(min(ref[0], ref[1]))
    assert 1 < n < 150 and ref[0] != ref[1], ref.tolist()
    free = _solve(b, num_iters=1, tol=1e-3)
    assert free["stats"][:2, 1].tolist() == ref[:2].tolist(), (free["stats"][:, 1].tolist(), ref.tolist())
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=1, tol=1e-3, maxit=n))
    print("maxit", n, "FISTA iterations (force, motion)", got["stats"][:, 1:3].tolist(), "without the cap", free["stats"][:, 1:3].tolist())
    assert got["stats"][:2, 1].tolist() == [n, n]
    assert np.all(got["cert_phases"][:, 0] == 1)


def test_floor_hand_over(hiplib, knobs):
    """tol = 1e-30: every certified loop runs until a step falls below the floor and hands the phase to the tested loop, which finds
    x_k and its image in LDS and the counts of the iterations done so far.  Three ADMM iterations of three problems; the force phases
    behind the first have no certificate at this tolerance, so each wave hands over four times.  The iteration a loop hands over at is in no output (the trace has the phase's total, the tested loop's share
    included), so that both copies of the loop -- an even and an odd index -- handed over cannot be asserted here; the comparison of
    `trace` with the build that keeps the shared loops covers whichever occurred."""
    b = problems.make_batch("solo12_trot", 3, H=20)
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3, tol=1e-30, maxit=4000))
    assert np.all(got["cert_phases"][:, 0] >= 1) and np.all(got["cert_phases"][:, 1] == 3)
    print("FISTA iterations per ADMM iteration (force, motion)", got["trace"][:, :, :2].tolist(), "retries", got["stats"][:, 3:5].tolist())


def test_a_diverged_wave_mate_stays_contained(hiplib, knobs):
    """problems 0 and 3 start at a velocity of 1e200 and are NaN after two ADMM iterations; problem 1 sits behind a diverged problem
    in its wave, problem 2 in front of one: both return the bits of the unpoisoned batch on every build (not cert_phases: a
    certificate is the wave's)"""
    clean = problems.make_batch("solo12_trot", 4, H=20)
    bad = problems.make_batch("solo12_trot", 4, H=20)
    bad.x_init[0, 3] = bad.x_init[3, 3] = 1e200
    ref = _builds(knobs, hiplib, clean, lambda: _solve(clean, num_iters=10))
    got = _builds(knobs, hiplib, bad, lambda: _solve(bad, num_iters=10))
    assert got["stats"][:, 5].tolist() == [2, 0, 0, 2]
    assert got["stats"][:, 0].tolist() == [2, 10, 10, 2]
    for i in (1, 2):
        for k in KEYS:
            assert np.all(np.isfinite(got[k][i])), (i, k)
            assert np.array_equal(got[k][i], ref[k][i]), (i, k)
