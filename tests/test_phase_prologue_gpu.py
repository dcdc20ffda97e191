"""The phase prologues of the loop-constants build ("Phase prologues"): outside its FISTA loops the kernel reads the
blocks of a lane's LDS record unconditionally, one batch per block behind one wait, from an address made where it is used, and keeps or
drops what it read with a select; the x_init rows come as one batch of global loads.  None of it may show in any output: every case
compares bmpc_set_loop_constants_in_lds 1 against 0 (the two-waves build, which keeps the masked reads) and against the one-wave build,
bit for bit, on X, F, P, stats, L_x, L_f, trace, hist and dyn_viol -- with the helpers of tests/test_loop_constants_gpu.py, as
tests/test_scalar_diet_gpu.py compares.  The shapes are those at which the prologues, not the loops, are what runs and what can go
wrong: B = 3 (a full wave and a half-empty one), few iterations, and horizons that leave 15, 14 and 11 lanes of a segment without a knot
-- the lanes whose unconditional reads land somewhere else."""
import numpy as np
import pytest

from bunmpc_amd import batch as bb
from bunmpc_amd import problems
from tests.test_loop_constants_gpu import HEADLINE, KEYS, ONE_WAVE, _builds, _solve, knobs  # noqa: F401  (knobs: the fixture)
from tests.util import launch_record

pytestmark = pytest.mark.gpu

HORIZONS = [16, 17, 20]      # 17, 18 and 21 knots in segments of 32 lanes


@pytest.mark.parametrize("H", HORIZONS)
def test_cold_starts(hiplib, knobs, H):
    b = problems.make_batch("solo12_trot", 3, H=H)
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3))
    assert np.all(got["stats"][:, 0] == 3) and np.all(got["stats"][:, 5] == 0)
    assert np.array_equal(got["cert_phases"], np.full((3, 2), 3))


@pytest.mark.parametrize("maxit", [1, 2])
@pytest.mark.parametrize("H", HORIZONS)
def test_cold_starts_that_are_almost_all_prologue(hiplib, knobs, H, maxit):
    """one or two FISTA iterations per phase: nearly every instruction executed is prologue, certificate or epilogue"""
    b = problems.make_batch("solo12_trot", 3, H=H)
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3, maxit=maxit))
    assert np.all(got["stats"][:, 1] == 3 * maxit) and np.all(got["stats"][:, 2] == 3 * maxit)
    assert np.all(got["stats"][:, 0] == 3) and np.all(got["stats"][:, 5] == 0)


@pytest.mark.parametrize("H", HORIZONS)
def test_warm_start_with_forces_and_multipliers(hiplib, knobs, H):
    """the F and P blocks that the prologues read are not zeros: a warm start from a solve's results, with the step constants it left"""
    b = problems.make_batch("solo12_trot", 3, H=H)
    c = _solve(b, num_iters=5)
    assert np.any(c["F"] != 0) and np.any(c["P"] != 0)
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3, warm=(c["X"], c["F"], c["P"]), L_x=c["L_x"], L_f=c["L_f"]))
    assert np.all(got["stats"][:, 0] == 3) and np.all(got["stats"][:, 5] == 0)
    assert not np.array_equal(got["P"], c["P"])      # (the multipliers' read-modify-write at the end of an ADMM iteration ran)


def test_iterates_reset_with_step_constants_carried(hiplib, knobs):
    """cold_start = 2: X = tile(x_init), F = P = 0 again, L_x and L_f as the caller carries them"""
    b = problems.make_batch("solo12_trot", 3, H=20)
    L_x, L_f = 1.5 * bb.L0_X, 1.5 * bb.L0_F      # (what a backtracking step of an earlier solve would have left)

    def solve():      # (the device path: the host entry point has no cold_start = 2; it records no cert_phases)
        dev = bb.DeviceBatch(b, num_iters=3, keep_hist=True)
        dev.set_step_constants(L_x, L_f)
        dev.cold_start(carry_step_constants=True)
        dev.solve()
        return dev.results()

    runs = {}
    for name, two_waves, clds, kernel in (("loop constants", 1, 1, HEADLINE), ("two waves", 1, 0, HEADLINE), ("one wave", 0, 0, ONE_WAVE)):
        knobs("bmpc_set_two_waves_per_simd", two_waves)
        knobs("bmpc_set_loop_constants_in_lds", clds)
        runs[name] = solve()
        assert launch_record(hiplib) == kernel, name
    for name in ("two waves", "one wave"):
        for k in KEYS:
            assert np.array_equal(runs["loop constants"][k], runs[name][k], equal_nan=True), (name, k)
    got = runs["loop constants"]
    assert np.all(got["stats"][:, 0] == 3) and np.all(got["stats"][:, 5] == 0)
    assert np.all(got["L_x"] >= L_x) and np.all(got["L_f"] >= L_f)      # (carried, not reset: a step constant never falls)


@pytest.mark.parametrize("H", HORIZONS)
def test_a_diverged_wave_mate_stays_contained(hiplib, knobs, H):
    """problems 0 and 3 start at a velocity of 1e200 and are NaN after two ADMM iterations; problem 1 sits behind a diverged problem in its
    wave, problem 2 in front of one -- on either side of a segment's end, where an idle lane's unconditional read or a wave shift finds
    the other problem's NaNs.  Both return the bits of their solve beside a healthy mate, on every build (not cert_phases: a certificate
    is the wave's)."""
    clean = problems.make_batch("solo12_trot", 4, H=H)
    bad = problems.make_batch("solo12_trot", 4, H=H)
    bad.x_init[0, 3] = bad.x_init[3, 3] = 1e200
    ref = _builds(knobs, hiplib, clean, lambda: _solve(clean, num_iters=4))
    got = _builds(knobs, hiplib, bad, lambda: _solve(bad, num_iters=4))
    assert got["stats"][:, 5].tolist() == [2, 0, 0, 2]
    assert got["stats"][:, 0].tolist() == [2, 4, 4, 2]
    for i in (1, 2):
        for k in KEYS:
            assert np.all(np.isfinite(got[k][i])), (i, k)
            assert np.array_equal(got[k][i], ref[k][i]), (i, k)


def test_a_horizon_that_does_not_fit_runs_the_two_waves_build(hiplib, knobs):
    """H = 21: the loop-constants build is refused and the two-waves build runs, unchanged"""
    b = problems.make_batch("solo12_trot", 3, H=21)
    assert hiplib.bmpc_loop_constants_fit(4, 21) == 0
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3), fits=False)
    assert np.all(got["stats"][:, 0] == 3) and np.all(got["stats"][:, 5] == 0)
