"""Stage 1 of the two-stage screen in the benchmark kernel's certified FISTA loops (biconvex_admm_body.h: kScreenTermsX / kScreenTermsF;
DESIGN.md section 4), restated in numpy on tools/screen_rate.py's theta, butterfly_sum32 and verdicts.  A lane's partial of |d|^2 is an
fma chain g over its 9 (motion) or 12 (force) squares; stage 1 takes the chain s over a FEW of them and asks s > theta.  The exact
sums are ordered, either chain rounds at most 12 times, so g >= s (1 - 2^-48); the segment sum S of the full partials in any order is at
least g; theta carries (1 + 2^-40) over max(tol^2, floor2) and is at least 2^-1000.  So whenever a lane's subset chain exceeds theta,
all three fp64 verdicts on the kernel-order sum of the FULL partials -- below the floor, done, inside the 1e-14 edge band -- are false.

The chains here ARE fma chains: every d is an integer below 2^26 times a power of two no smaller than 2^-537, so d * d is exact in
fp64 (subnormal results included) and fl(d * d + g) is fma(d, d, g)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import screen_rate as sr  # noqa: E402

from tests import lanes_np  # noqa: E402  (theta, butterfly_sum32: the models the device is held to)

# the kernel's own choice first (kScreenTermsX = {5}, kScreenTermsF = {8}), then the other sets DESIGN.md's table rates
SUBSETS = {9: [(5,), (3, 5), (3, 4, 5), (0,), (0, 8)], 12: [(8,), (2,), (2, 5), (2, 5, 8, 11), (0, 11)]}


def _exact_square_steps(x):
    """x >= 0 rounded down to m 2^u, m an integer below 2^26, u >= -537: its square is exact in fp64"""
    x = np.asarray(x, np.float64)
    with np.errstate(divide="ignore"):
        u = np.maximum(np.floor(np.log2(np.where(x > 0, x, 1.0))) - 25, -537)
    m = np.minimum(np.floor(np.ldexp(x, -u.astype(np.int64))), 2.0 ** 26 - 1)
    return np.ldexp(m, u.astype(np.int64))


def _steps(rng, n, nt, centre):
    """[n][32][nt] step components d: magnitudes over 20 decades below a per-row scale around `centre` (their squares: 40), with
    zero, subnormal-square, inf and NaN entries mixed in; returns (d, the rows' scales)"""
    scale = centre * 10.0 ** rng.uniform(-15, 5, size=(n, 1, 1))
    d = _exact_square_steps(scale * 10.0 ** rng.uniform(-20, 0, size=(n, 32, nt)))
    kind = rng.integers(0, 40, size=(n, 32, nt))
    d[kind == 0] = 0.0
    d[kind == 1] = np.ldexp(rng.integers(1, 2 ** 26, size=(n, 32, nt)).astype(np.float64), -537)[kind == 1]      # squares below 2^-1022
    lane_kind = rng.integers(0, 40, size=(n, 32, 1))
    d[np.broadcast_to((lane_kind == 2) & (rng.random((n, 1, 1)) < 0.05), d.shape) & (kind < 20)] = np.inf
    d[np.broadcast_to((lane_kind == 3) & (rng.random((n, 1, 1)) < 0.3), d.shape) & (kind < 10)] = np.nan
    d[rng.random(n) < 0.02] = 0.0      # (problems that do not move at all)
    d *= np.where(rng.random(d.shape) < 0.5, -1.0, 1.0)
    return d, scale[:, 0, 0]


def _chain(d, terms):
    """the kernel's chain over the named components in increasing order: g = fma(d, d, g) from g = 0 (d * d is exact here)"""
    g = np.zeros(d.shape[:-1])
    with np.errstate(invalid="ignore", over="ignore"):
        for j in terms:
            g = d[..., j] * d[..., j] + g
    return g


def _check(d, terms, tol2, floor2, label):
    nt = d.shape[-1]
    s, g = _chain(d, terms), _chain(d, range(nt))
    th = lanes_np.theta(tol2, floor2)
    assert np.all(th >= np.fmax(tol2, floor2)) and np.all(th >= 2.0 ** -1000)
    with np.errstate(invalid="ignore"):
        hit = np.any(s > th[:, None], axis=1)
        ok = np.isnan(s) | np.isnan(g) | (g >= s * (1.0 - 2.0 ** -48))      # the lemma between the two chains, lane by lane
    assert np.all(ok)
    S = lanes_np.butterfly_sum32(g)
    below, done, edge = sr.verdicts(S, tol2, floor2)
    with np.errstate(invalid="ignore"):
        full_hit = np.any(g > th[:, None], axis=1)
    print(label, "terms", terms, "of", nt, "| rows", len(S), "stage 1 settles", int(hit.sum()), "the whole partial", int(full_hit.sum()),
          "| settled rows with a NaN lane", int((hit & np.isnan(S)).sum()), "with an infinite sum", int((hit & np.isinf(S)).sum()),
          "| unsettled rows below the floor", int((~hit & below).sum()), "done", int((~hit & done).sum()), "edge", int((~hit & edge).sum()))
    assert not (hit & below).any()
    assert not (hit & done).any()
    assert not (hit & edge).any()
    return hit, S, below, done


def _thresholds(rng, s, scale2):
    """tol^2 and floor2 per row: half of them within 1e-16 .. 1e-1 (relative) of the row's largest subset chain -- where stage 1 is
    decided -- the others far from it, and the odd cases (zero, subnormal, infinite)"""
    n = len(scale2)
    with np.errstate(invalid="ignore"):
        smax = np.nanmax(np.where(np.isinf(s), 0.0, s), axis=1)
    near = np.where(smax > 0, smax, scale2)
    tol2 = near * np.where(rng.random(n) < 0.5, 1.0 + rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-16, -1, n), 10.0 ** rng.uniform(-12, 4, n))
    floor2 = near * np.where(rng.random(n) < 0.5, 1.0 + rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-16, -1, n), 10.0 ** rng.uniform(-30, 4, n))
    odd = rng.integers(0, 50, n)
    tol2[odd == 0] = 0.0
    floor2[odd == 1] = 0.0
    tol2[odd == 2] = 5e-324 * 3
    tol2[odd == 3] = 2.0 ** -1023
    floor2[odd == 4] = np.inf
    return tol2, floor2


@pytest.mark.parametrize("nt", [9, 12])
def test_a_subset_chain_above_theta_settles_every_fp64_verdict(nt):
    rng = np.random.default_rng(30 + nt)
    n = 30000
    d, scale = _steps(rng, n, nt, 1.0)
    for terms in SUBSETS[nt]:
        tol2, floor2 = _thresholds(rng, _chain(d, terms), scale * scale)
        hit, S, below, done = _check(d, terms, tol2, floor2, "ordinary")
        assert hit.sum() > n // 10 and (~hit).sum() > n // 10
        assert (hit & np.isnan(S)).any() and (~hit & (below | done)).any()


@pytest.mark.parametrize("nt", [9, 12])
def test_with_a_subnormal_tolerance(nt):
    """tol^2 subnormal (tol = 1e-160 and below): the relative margins round away and theta's lower limit 2^-1000 takes over; the steps
    lie around 2^-500, their squares from zero through the subnormals to well above 2^-1000"""
    rng = np.random.default_rng(40 + nt)
    n = 30000
    scale = 2.0 ** -500 * 10.0 ** rng.uniform(-6, 4, size=(n, 1, 1))
    d = _exact_square_steps(scale * 10.0 ** rng.uniform(-20, 0, size=(n, 32, nt)))
    d[rng.integers(0, 30, size=d.shape) == 0] = 0.0
    nanlane = (rng.integers(0, 40, size=(n, 32, 1)) == 0) & (rng.random((n, 1, 1)) < 0.3)
    d[np.broadcast_to(nanlane, d.shape)] = np.nan
    tol2 = 5e-324 * rng.integers(0, 2 ** 51, n).astype(np.float64)      # 0 .. 2^-1023, every one subnormal
    floor2 = np.where(rng.random(n) < 0.5, 0.0, 5e-324 * rng.integers(0, 2 ** 40, n).astype(np.float64))
    assert np.all(tol2 < 2.0 ** -1022)
    for terms in SUBSETS[nt]:
        hit, S, below, done = _check(d, terms, tol2, floor2, "subnormal tol^2")
        assert hit.sum() > n // 10 and (~hit).sum() > n // 10
        assert np.all(lanes_np.theta(tol2, floor2) == 2.0 ** -1000)


@pytest.mark.parametrize("nt", [9, 12])
def test_one_ulp_above_theta_with_every_other_term_zero(nt):
    """the adversarial case: one lane's subset terms alone are non-zero and their chain is ONE ulp above theta -- the full partial is
    that chain, the segment sum is that partial, and what keeps it out of the 1e-14 edge band is theta's 2^-40 alone"""
    rng = np.random.default_rng(50 + nt)
    n = 20000
    for terms in SUBSETS[nt]:
        d = np.zeros((n, 32, nt))
        lane = rng.integers(0, 32, n)
        for j in terms:
            d[np.arange(n), lane, j] = _exact_square_steps(10.0 ** rng.uniform(-140, 140, n) * 10.0 ** rng.uniform(-3, 0, n))
        s = _chain(d, terms)[np.arange(n), lane]
        assert np.all(np.isfinite(s) & (s > 2.0 ** -990))
        # tol^2 whose theta is the double just below s: theta is monotone in tol^2 and moves by about an ulp per ulp
        target = np.nextafter(s, 0.0)
        tol2 = np.full(n, np.nan)
        cand = s / (1.0 + 2.0 ** -40)
        for _ in range(4):
            cand = np.nextafter(cand, 0.0)
        for _ in range(9):
            tol2 = np.where((lanes_np.theta(cand, 0.0) == target) & np.isnan(tol2), cand, tol2)
            cand = np.nextafter(cand, np.inf)
        found = ~np.isnan(tol2)
        assert found.sum() > n // 2, found.sum()
        d, s, tol2 = d[found], s[found], tol2[found]
        floor2 = np.where(rng.random(len(s)) < 0.5, tol2, 0.0)      # (the floor at the same place, or out of the way)
        th = lanes_np.theta(tol2, floor2)
        assert np.all(s == np.nextafter(th, np.inf))
        hit, S, below, done = _check(d, terms, tol2, floor2, "one ulp above")
        assert hit.all() and np.array_equal(S, s)
