"""The priority rule of the SIMD-mate waves as the model of tests/simd_mates_np.py: its truth table, and what it does to two waves that
share a SIMD whose arbiter favours the older one (profiles/simd_mates_step0.txt).

The bound.  Under the rule the wave that has entered fewer phases holds the higher priority, so it advances at hi / (its phase cost)
phases per slot against lo / (the other's): it gains on its mate whenever the two waves' phase costs lie within hi / lo = 1.70 of each
other, and then the waves are never more than one phase boundary apart -- when the first finishes, its mate has at most the phase it is
in and one more to run, alone, at the lone rate >= 1: the finish times differ by at most TWO PHASES' WORTH, 2 x the largest phase cost.
Without the rule the older wave runs at hi throughout and the younger finishes its remainder alone: with equal work the older's time is
1 / (1 + (hi - lo) / lone) = 0.722 of the younger's, the ratio of the two mean wave lives that step 0 measured (1620 / 2244 us)."""
import numpy as np
import pytest

from bunmpc_amd import problems
from tests import simd_mates_np as sm


def test_truth_table():
    D = sm.DONE
    #          n  m  priority
    rows = [(1, 0, 0),      # the mate has published nothing yet
            (1, 1, 1),      # level: the mate published first
            (1, 2, 1),      # the mate is ahead
            (5, 4, 0),      # the mate is behind
            (5, 5, 1), (5, 20, 1),
            (1, D, 0), (20, D, 0),      # the mate has finished
            (D, 3, 0), (D, D, 0)]       # behind the last phase: priority 0 whatever the mate says
    for n, m, p in rows:
        assert sm.rule(n, m) == p, (n, m)


@pytest.fixture(scope="module")
def bench_waves(oracle):
    """phase costs of the 32 waves of the first 64 problems of the bench batch, from the strict oracle's per-phase counts"""
    b = problems.make_batch("solo12_trot", 4096).take(list(range(64)))
    tr = oracle.solve_batch(b, num_iters=10, trace=True)["trace"]
    it_f = np.diff(tr[:, :, 0], axis=1, prepend=0)
    it_x = np.diff(tr[:, :, 1], axis=1, prepend=0)
    assert it_f.min() >= 1 and it_x.min() >= 1
    return sm.wave_phase_costs(it_f, it_x)


def test_bench_waves_finish_together_under_the_rule(bench_waves):
    """SIMD-mates as the device pairs them, wave i with wave i + half the grid"""
    c = bench_waves
    half = len(c) // 2
    worst_on, off = 0.0, []
    for i in range(half):
        t0, t1 = sm.simulate(c[i], c[i + half])
        bound = 2.0 * max(c[i].max(), c[i + half].max())
        print("waves %2d / %2d: work %.0f / %.0f, finish with the rule %.0f / %.0f (bound on the difference %.0f)" % (i, i + half, c[i].sum(), c[i + half].sum(), t0, t1, bound))
        assert abs(t1 - t0) <= bound
        worst_on = max(worst_on, abs(t1 - t0) / max(t0, t1))
        u0, u1 = sm.simulate(c[i], c[i + half], rule_on=False)
        assert u1 > u0
        off.append((u1 - u0) / u1)
        assert max(t0, t1) < u1      # ... and the SIMD is done sooner
    print("younger - older over the SIMD's time: with the rule at most %.3f, without it %.3f .. %.3f" % (worst_on, min(off), max(off)))
    assert worst_on < 0.1
    assert 0.15 < min(off) and max(off) < 0.4      # (step 0 measured 0.22 .. 0.30 of the kernel time, 5th .. 95th percentile)


def test_random_sequences():
    """twenty phases per wave, costs within a factor 1.6 of each other (below hi / lo: see the bound)"""
    rng = np.random.default_rng(7)
    for _ in range(200):
        a, b = rng.uniform(100.0, 160.0, 20), rng.uniform(100.0, 160.0, 20)
        t0, t1 = sm.simulate(a, b)
        assert abs(t1 - t0) <= 2.0 * 160.0, (t0, t1)
        u0, u1 = sm.simulate(a, b, rule_on=False)
        assert u1 - u0 > 0.15 * u1
        f0, f1 = sm.simulate(a, b, rule_on=False, fair=True)      # an even arbiter has no such gap, with or without the rule
        assert abs(f1 - f0) <= abs(a.sum() - b.sum()) + 1e-6


def test_equal_work_without_the_rule_matches_step_0():
    w = np.full(20, 100.0)
    u0, u1 = sm.simulate(w, w, rule_on=False)
    assert u0 == pytest.approx(2000.0 / sm.HI)
    left = 2000.0 - sm.LO * u0      # the younger's remainder, alone at the lone rate
    assert u1 == pytest.approx(u0 + left / sm.LONE)
    assert u0 / u1 == pytest.approx(1620.0 / 2244.0, abs=0.005)
    t0, t1 = sm.simulate(w, w)
    assert max(t0, t1) == pytest.approx(2000.0, rel=0.03)      # level waves: the pair's throughput to the end
    assert max(t0, t1) < 0.92 * u1


def test_a_mate_that_never_publishes():
    """a wave that reads 0 at every boundary stays at priority 0: with both words silent, the times of the run without the rule; with
    one silent, the wave that does publish is never favoured over its mate and finishes no sooner than without the rule"""
    assert all(sm.rule(n, 0) == 0 for n in list(range(1, 41)) + [sm.DONE])
    a, b = np.full(20, 100.0), np.full(20, 120.0)
    off = sm.simulate(a, b, rule_on=False)
    assert sm.simulate(a, b, publishes=(False, False)) == pytest.approx(off)
    assert sm.simulate(a, b, publishes=(True, False))[0] >= off[0] - 1e-9
    assert sm.simulate(a, b, publishes=(False, True))[1] >= off[1] - 1e-9


def test_a_mate_that_finishes_at_phase_one():
    """its DONE lowers the other's priority at the next boundary; the other then runs alone"""
    a, b = np.full(20, 100.0), np.array([50.0])
    t0, t1 = sm.simulate(a, b)
    assert t1 < t0
    # wave 1 enters second and reads 1 >= 1: it holds the priority for its one phase
    assert t1 == pytest.approx(50.0 / sm.HI)
    assert t0 == pytest.approx(t1 + (2000.0 - sm.LO * t1) / sm.LONE)
    assert sm.simulate(b, a)[0] < sm.simulate(b, a)[1]
