"""The arithmetic behind the lane-local screen of the benchmark kernel's certified FISTA loops (biconvex_lanes.h: screen_theta; DESIGN.md
section 4), restated in numpy (tools/screen_rate.py): the fp64 sum of non-negative lane partials, in the kernel's butterfly order, is
at least its largest term, so one partial above theta = max(tol^2, floor2) (1 + 2^-40) makes all three fp64 verdicts of the iteration
-- below the floor, done, inside the 1e-14 edge band around tol^2 -- false, NaN lanes or not."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import screen_rate as sr  # noqa: E402

from tests import lanes_np  # noqa: E402  (theta, butterfly_sum32: the models the device is held to)


def _partials(rng, n):
    """[n][32] non-negative partials over 40 decades around a per-row scale, with zero, denormal, inf and NaN lanes mixed in"""
    scale = 10.0 ** rng.uniform(-30, 10, size=(n, 1))
    p = scale * 10.0 ** rng.uniform(-40, 0, size=(n, 32))
    kind = rng.integers(0, 40, size=(n, 32))
    p[kind == 0] = 0.0
    p[kind == 1] = 5e-324 * rng.integers(1, 1000, size=(n, 32))[kind == 1]
    p[(kind == 2) & (rng.random((n, 1)) < 0.05)] = np.inf
    p[(kind == 3) & (rng.random((n, 1)) < 0.3)] = np.nan
    p[rng.random(n) < 0.02] = 0.0      # (knots that do not move at all)
    return p, scale[:, 0]


def _thresholds(rng, p, scale):
    """(tol2, floor2) [n]: thresholds near the rows' own sizes (most of them at the largest partial, where the screen is decided), far from
    them, and the odd cases: zero, subnormal, infinite"""
    n = len(p)
    pmax = np.nanmax(np.where(np.isinf(p), 0.0, p), axis=1)
    near = np.where(pmax > 0, pmax, scale)
    tol2 = near * np.where(rng.random(n) < 0.5, 1.0 + rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-16, -1, n), 10.0 ** rng.uniform(-12, 4, n))
    floor2 = near * np.where(rng.random(n) < 0.5, 1.0 + rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-16, -1, n), 10.0 ** rng.uniform(-30, 4, n))
    odd = rng.integers(0, 50, n)
    tol2[odd == 0] = 0.0
    floor2[odd == 1] = 0.0
    tol2[odd == 2] = 5e-324 * 3
    tol2[odd == 3] = 2.0 ** -1023      # subnormal: the relative margins round away, the screen's lower limit takes over
    floor2[odd == 4] = np.inf
    return tol2, floor2


def test_a_partial_above_theta_settles_every_fp64_verdict():
    rng = np.random.default_rng(20)
    n = 200000
    p, scale = _partials(rng, n)
    tol2, floor2 = _thresholds(rng, p, scale)
    th = lanes_np.theta(tol2, floor2)
    assert np.all(th >= np.maximum(tol2, floor2)) and np.all(th >= 2.0 ** -1000)
    with np.errstate(invalid="ignore"):
        hit = np.any(p > th[:, None], axis=1)
    S = lanes_np.butterfly_sum32(p)
    below, done, edge = sr.verdicts(S, tol2, floor2)
    print("rows", n, "screened", int(hit.sum()), "of them with a NaN lane", int((hit & np.isnan(S)).sum()), "with an infinite sum",
          int((hit & np.isinf(S)).sum()), "| unscreened rows below the floor", int((~hit & below).sum()), "done", int((~hit & done).sum()),
          "edge", int((~hit & edge).sum()))
    assert hit.sum() > n // 10 and (~hit).sum() > n // 10
    assert (hit & np.isnan(S)).any() and (~hit & (below | done)).any()
    assert not (hit & below).any()
    assert not (hit & done).any()
    assert not (hit & edge).any()
    # the sum is at least its largest term whatever the order: the reverse butterfly and a plain left-to-right sum too
    with np.errstate(invalid="ignore", over="ignore"):
        for T in (lanes_np.butterfly_sum32(p[:, ::-1]), np.add.reduce(p, axis=1)):
            ok = np.isnan(T) | (T >= np.nanmax(p, axis=1))
            assert np.all(ok)


def test_screen_rate_on_four_trot_problems():
    from bunmpc_amd import problems
    b = problems.make_batch("solo12_trot", 4)
    r = sr.rates(b, range(4))
    for which in ("force", "motion"):
        hit, total = r[which]
        print(which, "wave-iterations", total, "screened", hit)
        assert 0 < hit < total
