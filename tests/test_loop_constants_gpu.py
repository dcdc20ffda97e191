"""The loop-constants build of the benchmark's kernel (bmpc_set_loop_constants_in_lds): its certified FISTA loops keep
x_k and its image in registers and read 18 constants of the phase from LDS, where the two-waves build keeps the constants in registers
and x_k in LDS.  Same operations in the same order, so nothing may show in any output: bit for bit (NaN-aware) mode 1 against mode 0
(the two-waves build) and against the one-wave build.  The record of the launch is the same for both two-waves builds; which one a
launch took is asked of bmpc_biconvex_plan_launch under the same switches.  (cert_phases is compared between the two builds that record
it; the one-wave build leaves it at -1.)"""
import ctypes as C

import numpy as np
import pytest

from bunmpc_amd import _lib
from bunmpc_amd import batch as bb
from bunmpc_amd import problems
from tests import dispatch_rows as dr
from tests.util import knob_setter, launch_record

pytestmark = pytest.mark.gpu

KEYS = ("X", "F", "P", "stats", "L_x", "L_f", "trace", "hist", "dyn_viol")
HEADLINE = ("biconvex_admm_kernel", 32, 2)
ONE_WAVE = ("biconvex_admm_kernel", 32, 1)


@pytest.fixture
def knobs():
    """sets dispatch knobs for one test and restores every one of them afterwards; small batches take the two-waves kernel"""
    with knob_setter() as set_:
        set_("bmpc_set_latency_mapping_max_batch", 0)
        set_("bmpc_set_three_per_wave", 0)
        set_("bmpc_set_two_waves_per_simd", 1)
        set_("bmpc_set_loop_constants_in_lds", 1)
        yield set_


def _planned(hiplib, b):
    """does a solve of b take the loop-constants build under the current switches?"""
    d, out = dr.descriptor(dict(E=b.E, k=b.H + 1, B=b.B, form="harness", precision=0, num_iters=10)), _lib.LaunchPlan()
    assert hiplib.bmpc_biconvex_plan_launch(C.byref(d), 0, 1024, C.byref(out)) == 0
    return out.loop_constants_in_lds


def _solve(b, **kw):
    got = bb.solve_host(b, keep_hist=True, cert_phases=True, **kw)
    assert all(k in got for k in KEYS + ("cert_phases",)), sorted(got)
    return got


def _same(a, b, what, cert=True):
    for k in KEYS + (("cert_phases",) if cert else ()):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _builds(knobs, hiplib, b, solve, fits=True):
    """solve() on the loop-constants build (the returned run), on the two-waves build and on the one-wave build: every output equal"""
    knobs("bmpc_set_two_waves_per_simd", 1)
    knobs("bmpc_set_loop_constants_in_lds", 1)
    assert _planned(hiplib, b) == (1 if fits else 0)
    new = solve()
    assert launch_record(hiplib) == HEADLINE
    knobs("bmpc_set_loop_constants_in_lds", 0)
    assert _planned(hiplib, b) == 0
    old = solve()
    assert launch_record(hiplib) == HEADLINE
    _same(new, old, "the two-waves build")
    knobs("bmpc_set_two_waves_per_simd", 0)
    one = solve()
    assert launch_record(hiplib) == ONE_WAVE
    assert np.all(one["cert_phases"] == -1)
    _same(new, one, "the one-wave build", cert=False)
    knobs("bmpc_set_two_waves_per_simd", 1)
    knobs("bmpc_set_loop_constants_in_lds", 1)
    return new


@pytest.mark.parametrize("H", [20, 16])
def test_cold_starts(hiplib, knobs, H):
    """B = 3: a full wave and a wave with one problem and a padding segment; H = 20 is the benchmark's segment, H = 16 the shortest that
    gets 32 lanes.  Every phase of these cold starts has its certificate, so both new loops ran in all three ADMM iterations."""
    b = problems.make_batch("solo12_trot", 3, H=H)
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3))
    assert np.all(got["stats"][:, 0] == 3) and np.all(got["stats"][:, 5] == 0)
    assert np.array_equal(got["cert_phases"], np.full((3, 2), 3))


def test_warm_start(hiplib, knobs):
    """a cold start, then a warm start from its results with the step constants it left behind"""
    b = problems.make_batch("solo12_trot", 4, H=20)
    c = _solve(b, num_iters=10)
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=4, warm=(c["X"], c["F"], c["P"]), L_x=c["L_x"], L_f=c["L_f"]))
    print("warm start: certified phases (force, motion) per problem", got["cert_phases"].tolist(), "ADMM iterations", got["stats"][:, 0].tolist())


def test_every_phase_leaves_by_the_iteration_cap(hiplib, knobs):
    """maxit = 3: no problem finishes a phase, every phase ends at iteration maxit - 1 -- the last iteration's store"""
    b = problems.make_batch("solo12_trot", 3, H=20)
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3, maxit=3))
    assert np.all(got["stats"][:, 1] == 9) and np.all(got["stats"][:, 2] == 9)
    assert np.array_equal(got["cert_phases"], np.full((3, 2), 3))


def test_wave_mates_finish_at_different_iterations(hiplib, knobs, oracle):
    """two problems of the perturbed batch whose iteration counts differ on the CPU oracle, in one wave: the one that finishes a phase
    first is latched while its wave-mate goes on"""
    six = problems.make_batch("solo12_trot", 6, H=20)
    ref = oracle.solve_batch(six, num_iters=3, tol=1e-3, trace=True)["trace"][:, -1, :2]
    pairs = [(i, j) for i in range(6) for j in range(i + 1, 6) if ref[i, 0] != ref[j, 0] or ref[i, 1] != ref[j, 1]]
    assert pairs, ref.tolist()
    b = six.take(list(pairs[0]))
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3, tol=1e-3))
    print("problems", pairs[0], "FISTA iterations (force, motion)", got["stats"][:, 1:3].tolist(), "certified phases", got["cert_phases"].tolist())
    assert got["stats"][0, 1:3].tolist() != got["stats"][1, 1:3].tolist()
    assert np.all(got["cert_phases"] > 0)


def test_a_diverged_wave_mate_stays_contained(hiplib, knobs):
    """problems 0 and 3 start at a velocity of 1e200 and are NaN after two ADMM iterations; problems 1 and 2 share their waves -- 1 behind
    a diverged problem, 2 in front of one -- and return the bits of the unpoisoned batch, on every build"""
    clean = problems.make_batch("solo12_trot", 4, H=20)
    bad = problems.make_batch("solo12_trot", 4, H=20)
    bad.x_init[0, 3] = bad.x_init[3, 3] = 1e200
    ref = _builds(knobs, hiplib, clean, lambda: _solve(clean, num_iters=10))
    got = _builds(knobs, hiplib, bad, lambda: _solve(bad, num_iters=10))
    assert got["stats"][:, 5].tolist() == [2, 0, 0, 2]
    assert got["stats"][:, 0].tolist() == [2, 10, 10, 2]
    for i in (1, 2):      # (not cert_phases: a certificate is the wave's, and a diverged wave-mate's phase has none)
        for k in KEYS:
            assert np.all(np.isfinite(got[k][i])), (i, k)
            assert np.array_equal(got[k][i], ref[k][i]), (i, k)


def test_floor_hand_over(hiplib, knobs):
    """tol far below machine precision: the certified loops run until their steps fall below the floor and hand the phase to the tested
    loop, which finds x_k and its image in LDS"""
    b = problems.make_batch("solo12_trot", 2, H=20)
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=1, tol=1e-30, maxit=4000))
    assert np.array_equal(got["cert_phases"], np.ones((2, 2), int))
    print("FISTA iterations (force, motion)", got["stats"][:, 1:3].tolist(), "retries", got["stats"][:, 3:5].tolist())


@pytest.mark.parametrize("switch,value", [("bmpc_set_certified_steps", v) for v in (0, 1, 2)] + [("bmpc_set_exact_step_decisions", v) for v in (0, 1, 2)])
def test_switches(hiplib, knobs, switch, value):
    b = problems.make_batch("solo12_trot", 3, H=20)
    knobs("bmpc_set_certified_steps", 1)
    knobs("bmpc_set_exact_step_decisions", 0)
    base = _solve(b, num_iters=3)
    knobs(switch, value)
    got = _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3))
    _same(base, got, "%s %d" % (switch, value), cert=switch != "bmpc_set_certified_steps")
    expect = {0: [0, 0], 1: [3, 3], 2: [3, 0]}[value] if switch == "bmpc_set_certified_steps" else [3, 3]
    assert np.array_equal(got["cert_phases"], np.tile(expect, (3, 1)))


def test_refusal_falls_back_to_the_two_waves_build(hiplib, knobs):
    """H = 21: 22 knots' constants do not fit beside the records of two problems; mode 1 launches the two-waves build"""
    b = problems.make_batch("solo12_trot", 3, H=21)
    assert hiplib.bmpc_loop_constants_fit(4, 21) == 0 and hiplib.bmpc_loop_constants_fit(4, 20) == 1
    _builds(knobs, hiplib, b, lambda: _solve(b, num_iters=3), fits=False)


@pytest.mark.parametrize("H", [16, 20])
def test_eight_waves_are_resident_per_cu(hiplib, H):
    """two waves per SIMD: the occupancy query of the loaded kernel with the LDS of this horizon (at H = 20 eight waves' LDS is the CU's
    160 KB to the allocation granule)"""
    assert hiplib.bmpc_loop_constants_resident_waves(H) == 8
    assert hiplib.bmpc_loop_constants_resident_waves(21) == -1
