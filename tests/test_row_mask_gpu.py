"""The certified motion loop of the benchmark's kernel (biconvex_admm_kernel<double, 32, 4, false, false, 2>) without
its row mask, and the two-stage screen of both certified loops.  The loop no longer zeroes the image A_f x+ in lanes without a
dynamics row; it leaves their `ry` and their R block alone instead, so the rows that exist take the same operations in the same order.
Stage 1 of the screen asks one square of the lane's step what the whole partial would be asked.  Neither may show in any output: bit
for bit (NaN-aware) the certified loops against the tested ones (bmpc_set_certified_steps 2 and 0 run the motion step in the tested
loop, which keeps the mask), against the one-wave build, and under every value of bmpc_set_exact_step_decisions."""
import numpy as np
import pytest

from bunmpc_amd import batch as bb
from bunmpc_amd import problems
from tests.util import knob_setter, launch_record

pytestmark = pytest.mark.gpu

KEYS = ("X", "F", "P", "L_x", "L_f", "stats", "trace", "hist", "dyn_viol")
HEADLINE = ("biconvex_admm_kernel", 32, 2)
ONE_WAVE = ("biconvex_admm_kernel", 32, 1)


@pytest.fixture
def knobs():
    """sets dispatch knobs for one test and restores every one of them afterwards; the headline kernel is forced unless a test asks for
    the one-wave build"""
    with knob_setter() as set_:
        set_("bmpc_set_latency_mapping_max_batch", 0)
        set_("bmpc_set_three_per_wave", 0)
        set_("bmpc_set_two_waves_per_simd", 1)
        yield set_


def _solve(b, **kw):
    got = bb.solve_host(b, keep_hist=True, cert_phases=True, **kw)
    assert all(k in got for k in KEYS), sorted(got)
    return got


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _variants(knobs, hiplib, solve, lanes=32):
    """solve() on the headline kernel with both certified loops and the screen (the returned run), then with the motion step (value 2)
    and both steps (0) in the tested loops, on the one-wave build, and under the other two values of the decision switch: every
    output equal to the first run's.  lanes = 16: the kernel the dispatch gives a horizon of up to 15 knots (see test_cold_starts)."""
    two_waves, one_wave = (HEADLINE[0], lanes, 2), (ONE_WAVE[0], lanes, 1)
    knobs("bmpc_set_certified_steps", 1)
    knobs("bmpc_set_exact_step_decisions", 0)
    base = solve()
    assert launch_record(hiplib) == two_waves
    for v in (2, 0):
        knobs("bmpc_set_certified_steps", v)
        got = solve()
        assert launch_record(hiplib) == two_waves
        assert np.all(got["cert_phases"][:, 1] == (0 if lanes == 32 else -1))      # (the motion step ran the tested loop)
        _same(base, got, "certified_steps %d" % v)
    knobs("bmpc_set_certified_steps", 1)
    knobs("bmpc_set_two_waves_per_simd", 0)
    got = solve()
    assert launch_record(hiplib) == one_wave
    _same(base, got, "one wave per SIMD")
    knobs("bmpc_set_two_waves_per_simd", 1)
    for v in (1, 2):
        knobs("bmpc_set_exact_step_decisions", v)
        got = solve()
        assert launch_record(hiplib) == two_waves
        assert np.array_equal(got["cert_phases"], base["cert_phases"])
        _same(base, got, "exact_step_decisions %d" % v)
    knobs("bmpc_set_exact_step_decisions", 0)
    return base


@pytest.mark.parametrize("H,B", [(31, 3), (21, 2), (3, 5), (16, 5), (20, 5)])
def test_cold_starts(hiplib, knobs, H, B):
    """H = 31: every lane owns a knot and lane 31 is knot H, next to the wave-mate's knot 0; H = 16: the shortest horizon the dispatch
    gives 32-lane segments, 15 idle lanes per segment; B odd: a padding segment.  Every phase of these cold starts has its certificate
    (tools/certify_rate.py says so on the CPU oracle, with 4 % of margin), so both certified loops ran in all ten ADMM iterations.
    H = 3 was meant to leave 28 lanes of a 32-lane segment idle, but up to 15 knots the dispatch launches the 16-lane kernel, which no
    knob overrides and which has neither change; the case stays, held to the same equalities on that kernel (12 idle lanes per
    segment, no certificate telemetry), and H = 16 stands in for it on the headline kernel."""
    b = problems.make_batch("solo12_trot", B, H=H)
    got = _variants(knobs, hiplib, lambda: _solve(b, num_iters=10), lanes=16 if H == 3 else 32)
    assert np.all(got["stats"][:, 0] == 10) and np.all(got["stats"][:, 5] == 0)
    assert np.array_equal(got["cert_phases"], np.full((B, 2), -1 if H == 3 else 10))


def test_warm_start(hiplib, knobs):
    """a cold start, then a warm start from its results with the step constants it left behind"""
    b = problems.make_batch("solo12_trot", 5, H=20)
    knobs("bmpc_set_certified_steps", 1)
    c = _solve(b, num_iters=10)
    got = _variants(knobs, hiplib, lambda: _solve(b, num_iters=4, warm=(c["X"], c["F"], c["P"]), L_x=c["L_x"], L_f=c["L_f"]))
    print("warm start: certified phases (force, motion) per problem", got["cert_phases"].tolist(), "ADMM iterations", got["stats"][:, 0].tolist())


def test_floor_hand_over_with_a_full_segment(hiplib, knobs):
    """tol far below machine precision and H = 31: the motion loop runs until its steps fall below the floor and hands the phase to the
    tested loop, which reads the R block of lane 31 (knot H) -- the zeros the certified loop never wrote over"""
    b = problems.make_batch("solo12_trot", 2, H=31)
    got = _variants(knobs, hiplib, lambda: _solve(b, num_iters=1, tol=1e-30, maxit=4000))
    assert np.array_equal(got["cert_phases"], np.ones((2, 2), int))
    print("FISTA iterations (force, motion)", got["stats"][:, 1:3].tolist(), "retries", got["stats"][:, 3:5].tolist())


@pytest.mark.parametrize("H", [31, 20])
def test_a_diverged_wave_mate_stays_contained(hiplib, knobs, H):
    """problems 0 and 3 start at a velocity of 1e200 and are NaN after two ADMM iterations (status 2, as on the CPU oracle); problems 1
    and 2 share their waves -- 1 behind a diverged problem (its lane 0 shifts in from lane 31), 2 in front of one (its last lane shifts
    in from lane 32) -- and must return the bits of the unpoisoned batch under every value of the decision switch"""
    clean = problems.make_batch("solo12_trot", 4, H=H)
    bad = problems.make_batch("solo12_trot", 4, H=H)
    bad.x_init[0, 3] = bad.x_init[3, 3] = 1e200
    knobs("bmpc_set_certified_steps", 1)
    for v in (0, 1, 2):
        knobs("bmpc_set_exact_step_decisions", v)
        ref = _solve(clean, num_iters=10)
        got = _solve(bad, num_iters=10)
        assert launch_record(hiplib) == HEADLINE
        print("switch", v, "H", H, "statuses", got["stats"][:, 5].tolist(), "ADMM iterations", got["stats"][:, 0].tolist(),
              "certified phases (force, motion)", got["cert_phases"].tolist())
        assert got["stats"][:, 5].tolist() == [2, 0, 0, 2]
        assert got["stats"][:, 0].tolist() == [2, 10, 10, 2]
        for i in (1, 2):
            for k in KEYS:
                assert np.all(np.isfinite(got[k][i])), (v, i, k)
                assert np.array_equal(got[k][i], ref[k][i]), (v, i, k)
