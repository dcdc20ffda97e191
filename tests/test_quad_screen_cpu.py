"""The margin of the quad stage of the screen (biconvex_lanes.h: quad_screen; the model: tests/quad_screen_np.py), held against exact
rational sums.  The stage may settle an iteration only if the EXACT sum Q of the quad's four non-negative partials satisfies
Q > theta (1 + 2^-22): the segment sum as the kernel adds it in fp64 -- five levels of additions of non-negative terms, each rounded to
nearest -- is then at least Q (1 - 2^-50) > max(tol^2, floor2) (1 + 2^-40) (1 + 2^-23), above the floor, above tol^2 and outside the
1e-14 band around it, which is what a single lane above theta settles (tests/test_step_decisions_cpu.py, tests/lanes_np.py).  So no
decision changes.  The other direction -- how often the stage fires -- is a matter of speed alone (tools/screen_rate.py --quad)."""
from fractions import Fraction

import numpy as np
import pytest

from tests import quad_screen_np as qs
from tests.lanes_np import seg_sum

SAFE = 1 + Fraction(1, 2 ** 22)


def _sound(quads, theta):
    """every quad [n, 4] that the model settles has an exact sum above theta (1 + 2^-22); returns how many it settled"""
    hit = qs.quad_screen(quads, theta)
    assert np.array_equal(hit, np.repeat(hit[:, :1], 4, axis=1)), "the four lanes of a quad hold the same sum"
    n = 0
    for row, h in zip(quads, hit[:, 0]):
        if h:
            n += 1
            assert sum(Fraction(float(v)) for v in row) > Fraction(float(theta)) * SAFE, (row.tolist(), theta)
    return n


def _thetas(rng, n):
    return [float(t) for t in np.concatenate([[1e-10, 1e-6, 9e-8, 2.0 ** -1000, 2.0 ** -126, 2.0 ** -100, 1e30, 3e38, 1e39, 1e300],
                                              10.0 ** rng.uniform(-40, 38, n)])]


def test_random_quads():
    rng = np.random.default_rng(1)
    fired = 0
    for theta in _thetas(rng, 30):
        scale = theta * 10.0 ** rng.uniform(-3, 1, (400, 1))
        fired += _sound(scale * rng.random((400, 4)) ** rng.integers(1, 6), theta)
    assert fired > 1000      # (the property is not vacuous)


@pytest.mark.parametrize("shape", ["equal", "dominant", "two", "ramp"])
def test_quads_at_the_threshold(shape):
    """sums within a few fp32 ulps of the threshold on either side, in the shapes that round worst: four equal lanes, one dominant
    lane with three tiny ones, two halves, a ramp -- every partial stepped by single fp64 ulps"""
    rng = np.random.default_rng(2)
    w = {"equal": [0.25, 0.25, 0.25, 0.25], "dominant": [1 - 3e-9, 1e-9, 1e-9, 1e-9], "two": [0.5, 0.5, 0.0, 0.0], "ramp": [0.1, 0.2, 0.3, 0.4]}[shape]
    fired = missed = 0
    for theta in _thetas(rng, 10):
        thq = float(qs.quad_theta(theta))
        if not np.isfinite(thq):
            assert not qs.quad_screen(np.full((1, 4), 1e300), theta).any()
            continue
        for rel in np.concatenate([np.linspace(-8, 8, 65) * 2.0 ** -24, rng.uniform(-1, 1, 40) * 2.0 ** -20]):
            base = np.array(w) * thq * (1.0 + rel)
            rows = []
            for _ in range(8):      # (neighbouring doubles: the conversion's ties)
                rows.append(base.copy())
                base = np.nextafter(base, np.inf)
            quads = np.array(rows)
            n = _sound(quads, theta)
            fired += n
            missed += len(quads) - n
    assert fired > 100 and missed > 100


def test_subnormals_and_zeros():
    """partials that are subnormal in fp32, or zero: the fp32 sum stays below the threshold's floor of 2^-100 whatever theta is"""
    rng = np.random.default_rng(3)
    tiny = 2.0 ** rng.uniform(-160, -127, (200, 4))
    tiny[::3, 1] = 0.0
    for theta in (2.0 ** -1000, 2.0 ** -200, 2.0 ** -140, 2.0 ** -126):
        assert _sound(tiny, theta) == 0
    mixed = tiny.copy()
    mixed[:, 0] = 2.0 ** rng.uniform(-101, -99, 200)      # one normal lane around the floor of the threshold
    for theta in (2.0 ** -1000, 2.0 ** -101, 2.0 ** -100):
        _sound(mixed, theta)


def test_nan_inf_and_the_switch():
    """theta = +inf (the screen switched off) settles nothing; a NaN partial settles nothing in its own quad and nothing changes in
    the next; an infinite partial is above every finite theta, as is the fp64 sum"""
    g = np.array([[1.0, 1.0, 1.0, 1.0, np.nan, 1.0, 1.0, 1.0]])
    assert not qs.quad_screen(g, np.inf).any()
    hit = qs.quad_screen(g, 1e-10)[0]
    assert hit[:4].all() and not hit[4:].any()
    assert qs.quad_screen(np.array([[np.inf, 0.0, 0.0, 0.0]]), 1e30).all()
    assert qs.quad_screen(np.array([[1e39, 1e39, 0.0, 0.0]]), 3.4e38).all()      # (q overflows to +inf above a finite threshold: the exact sum is above theta too)
    assert not qs.quad_screen(np.array([[1e39, 1e39, 0.0, 0.0]]), 3.5e38).any()      # (the threshold itself overflows fp32: +inf, above which nothing is)


@pytest.mark.parametrize("lanes_used", [21, 28, 32])
def test_a_settled_quad_means_a_clear_fp64_segment_sum(lanes_used):
    """end to end on 32-lane segments: where some quad settles, the kernel's own fp64 segment sum (tests/lanes_np.py: seg_sum) is
    above max(tol^2, floor2) (1 + 2^-40) (1 + 2^-23) -- no hand-over, no exit, not in the band around tol^2"""
    rng = np.random.default_rng(4 + lanes_used)
    tol2 = 1e-10
    theta = tol2 * (1.0 + 2.0 ** -40)
    settled = 0
    for _ in range(300):
        p = np.zeros(32)
        p[:lanes_used] = rng.random(lanes_used) ** 3 * tol2 * 10.0 ** rng.uniform(-2, 0.5)
        if qs.quad_screen(p[None, :], theta).any():
            settled += 1
            S = seg_sum(p[None, :].repeat(2, 0).reshape(1, 64), 32)[0, 0]
            assert Fraction(float(S)) > Fraction(theta) * (1 + Fraction(1, 2 ** 23))
            assert not (S < tol2) and not (abs(S - tol2) <= 1e-14 * tol2)
    assert settled > 50


def test_a_settled_quad_of_units_means_a_clear_fp64_segment_sum():
    """the force loop with two feet per lane: the stage sums a quad of UNIT lanes, each holding the fma chain over its own (at most six)
    squares, while the unsettled path sums the KNOTS' values -- the first unit's chain continued by the second's, twelve terms, brought
    to the knot's lane -- over the segment.  Another association of the same non-negative squares: a square passes through at most 12
    roundings of a chain and 5 of the segment sum there, and at most 6 in the unit's own chain, so the segment sum is at least
    Q (1 - 23 x 2^-53) for the exact sum Q of the quad's unit partials: still far inside the stage's margin of 2^-22"""
    from tests import foot_pairs_np as fp
    rng = np.random.default_rng(9)
    tol2 = 1e-10
    theta = tol2 * (1.0 + 2.0 ** -40)
    settled = 0
    for _ in range(150):
        masks = [int(rng.choice([0, 3, 5, 6, 9, 10, 12, 7, 11, 13, 14, 15], p=[.04, .1, .1, .1, .1, .1, .1, .05, .05, .05, .05, .16])) for _ in range(20)]
        units = fp.unit_map(masks)
        if len(units) > 32:
            continue
        d = rng.normal(size=(20, 4, 3)) * np.sqrt(tol2) * 10.0 ** rng.uniform(-1.5, 0)
        own = np.zeros(32)      # the units' own partials, on the unit lanes
        knot = np.zeros(32)     # the knots' chained values, on the knot lanes
        for lane, (t, rank, feet) in enumerate(units):
            sq = [d[t, n, k] for n in feet for k in range(3)] + [0.0] * (6 - 3 * len(feet))
            g = 0.0
            for v in sq:
                g = fp.fma(v, v, g)
            own[lane] = g
            gk = knot[t] if rank else 0.0      # (the second unit continues the first's chain)
            for v in sq:
                gk = fp.fma(v, v, gk)
            knot[t] = gk
        if qs.quad_screen(own[None, :], theta).any():
            settled += 1
            S = seg_sum(np.tile(knot, 2)[None, :], 32)[0, 0]
            assert Fraction(float(S)) > Fraction(theta) * (1 + Fraction(1, 2 ** 23))
            assert not (S < tol2) and not (abs(S - tol2) <= 1e-14 * tol2)
    assert settled > 30
