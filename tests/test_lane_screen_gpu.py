"""The lane-local screen of the benchmark's kernel (biconvex_admm_kernel<double, 32, 4, false, false, 2>): in a
certified FISTA loop a lane whose own share of |d|^2 is above max(tol^2, floor) (1 + 2^-40) settles, for its problem, that the step is
neither below the floor nor an exit -- the segment sum is at least its largest term -- so the iteration takes no sum at all.  The
decisions are the ones the fp64 sums make, so bmpc_set_exact_step_decisions 0 (screen, then fp32 decisions), 1 (fp64 sums only) and 2
(fp32 decisions, no screen) must not show in any output, bit for bit and NaN-aware."""
import numpy as np
import pytest

from bunmpc_amd import batch as bb
from bunmpc_amd import problems
from tests.util import TOL_FP64 as TOL, knob_setter, launch_record, rel_l2      # TOL: what tests/test_biconvex_gpu.py holds solo12_trot to

pytestmark = pytest.mark.gpu

KEYS = ("X", "F", "P", "L_x", "L_f", "stats", "trace", "hist", "dyn_viol", "cert_phases")
HEADLINE = ("biconvex_admm_kernel", 32, 2)


@pytest.fixture
def knobs():
    """sets dispatch knobs for one test and restores every one of them afterwards; the headline kernel is forced for every launch"""
    with knob_setter() as set_:
        set_("bmpc_set_latency_mapping_max_batch", 0)
        set_("bmpc_set_three_per_wave", 0)
        set_("bmpc_set_two_waves_per_simd", 1)
        yield set_


def _switches(knobs, hiplib, solve, values=(0, 1, 2)):
    """solve() under every value of the switch: the headline kernel each time, every output equal to the first value's"""
    out = {}
    for v in values:
        knobs("bmpc_set_exact_step_decisions", v)
        out[v] = solve()
        assert launch_record(hiplib) == HEADLINE
    for v in values[1:]:
        for k in KEYS:
            assert np.array_equal(out[values[0]][k], out[v][k], equal_nan=True), (v, k)
    return out


def _solve(b, **kw):
    got = bb.solve_host(b, keep_hist=True, cert_phases=True, **kw)
    assert all(k in got for k in KEYS), sorted(got)
    return got


def test_cold_and_warm_starts(hiplib, knobs):
    """five problems (the last wave holds one problem and one padding segment): a cold start, then a warm start from its results with
    the step constants it left behind; every phase of the cold start ran its certified loop"""
    b = problems.make_batch("solo12_trot", 5)
    cold = _switches(knobs, hiplib, lambda: _solve(b, num_iters=10))
    assert np.all(cold[0]["stats"][:, 0] == 10)
    assert np.array_equal(cold[0]["cert_phases"], np.full((5, 2), 10))
    c = cold[0]
    _switches(knobs, hiplib, lambda: _solve(b, num_iters=4, warm=(c["X"], c["F"], c["P"]), L_x=c["L_x"], L_f=c["L_f"]))


@pytest.mark.parametrize("H,B", [(31, 3), (21, 2)])
def test_horizons(hiplib, knobs, H, B):
    """H = 31: every lane of a segment owns a knot; H = 21: the first horizon that needs 32-lane segments"""
    b = problems.make_batch("solo12_trot", B, H=H)
    got = _switches(knobs, hiplib, lambda: _solve(b, num_iters=10))
    assert np.all(got[0]["cert_phases"] >= 0)


def test_early_exits(hiplib, knobs):
    """tol = 1e-3: the exits fire early, and wave-mates finish at different iterations (one problem of the wave screened alone)"""
    b = problems.make_batch("solo12_trot", 6)
    got = _switches(knobs, hiplib, lambda: _solve(b, num_iters=10, tol=1e-3))
    per = got[0]["stats"][:, 1:3]
    print("FISTA iterations (force, motion) per problem", per.tolist())
    assert np.any(per < 10 * 150) and len({tuple(r) for r in per.tolist()}) > 1      # (an exit fired; the problems differ)


def test_floor_governs_theta(hiplib, knobs):
    """tol far below machine precision: floor2 > tol^2, so the floor sets theta, the motion FISTA runs until its steps vanish, and the
    hand-over to the tested loop happens at the same iteration under every value -- with the bits and the iteration counts of value 1"""
    b = problems.make_batch("solo12_trot", 2)
    got = _switches(knobs, hiplib, lambda: _solve(b, num_iters=1, tol=1e-30, maxit=4000))
    assert np.array_equal(got[1]["cert_phases"], np.ones((2, 2), int))
    for v in (0, 2):
        assert np.array_equal(got[v]["stats"][:, 1:5], got[1]["stats"][:, 1:5])
    print("motion FISTA iterations", got[1]["stats"][:, 2].tolist(), "force", got[1]["stats"][:, 1].tolist())


def test_divergence(hiplib, knobs):
    """Go2 at the reference's mu = 1 diverges (NaN) on some problems -- NaN lanes in the screen's comparison: alike under every value
    of the switch, and a diverged problem's wave-mate keeps the bits it has under value 1"""
    b = problems.make_batch("go2_bound", 8, H=20)
    got = _switches(knobs, hiplib, lambda: _solve(b, num_iters=10, mu=1.0))
    bad = got[1]["stats"][:, 5] == 2
    assert bad.any()
    mates = [i ^ 1 for i in np.flatnonzero(bad) if not bad[i ^ 1]]
    print("diverged", np.flatnonzero(bad).tolist(), "wave-mates that did not", mates)
    for v in (0, 2):
        assert np.array_equal(got[v]["stats"][:, 5] == 2, bad)
        for i in mates:
            for k in ("X", "F", "P"):
                assert np.all(np.isfinite(got[v][k][i])) and np.array_equal(got[v][k][i], got[1][k][i])


def test_oracle_comparison(hiplib, knobs, oracle):
    """five problems under the screen against the strict CPU oracle: the discrete path per ADMM iteration, X and F"""
    b = problems.make_batch("solo12_trot", 5)
    ref = oracle.solve_batch(b, num_iters=10, trace=True)
    got = _switches(knobs, hiplib, lambda: _solve(b, num_iters=10), values=(0,))[0]
    assert np.array_equal(got["trace"], ref["trace"])
    for k in ("X", "F"):
        err = rel_l2(got[k], ref[k])
        print(k, "rel-L2 against the oracle", err)
        assert np.all(err < TOL), (k, err)
