"""tests/util.py::assert_matches_twin, the per-problem check every cost-shape kernel is held to, on a synthetic batch of three
problems: what it accepts and what it refuses.  No GPU and no library."""
import numpy as np
import pytest

from tests.util import K_SPREAD, TOL_FP64, assert_matches_twin, rel_l2


def _twins():
    rng = np.random.default_rng(20251020)
    return [dict(X=rng.normal(size=36), F=rng.normal(size=24), P=rng.normal(size=36), L_x=2.25e6, L_f=506.25 * 1.5 ** i,
                 stats=np.array([3, 40 + i, 50, i, 1, 0])) for i in range(3)]


def _got(twins):
    return {k: np.stack([np.array(r[k]) for r in twins]) for k in twins[0]}


def _moved(v, rel):
    """v moved by rel x |v| along a fixed direction: rel_l2(_moved(v, rel), v) = rel"""
    u = np.cos(np.arange(v.size))
    return v + rel * np.linalg.norm(v) * u / np.linalg.norm(u)


def _refused(got, twins, **kw):
    with pytest.raises(AssertionError):
        assert_matches_twin(got, twins, **kw)


def test_equal_results_pass_and_the_retries_are_returned():
    twins = _twins()
    assert assert_matches_twin(_got(twins), twins) == sum(r["stats"][3] + r["stats"][4] for r in twins) == 6


def test_one_count_off_by_one_is_refused():
    twins = _twins()
    for col in range(6):
        got = _got(twins)
        got["stats"][1, col] += 1
        _refused(got, twins)


def test_a_step_constant_off_by_one_ulp_is_refused():
    twins = _twins()
    for k in ("L_f", "L_x"):
        got = _got(twins)
        got[k][2] = np.nextafter(got[k][2], np.inf)
        _refused(got, twins)


def test_the_bound_on_the_iterates():
    twins = _twins()
    for k in "XFP":
        got = _got(twins)
        got[k][0] = _moved(got[k][0], 0.5 * TOL_FP64)
        assert rel_l2(got[k][0], twins[0][k]) == pytest.approx(0.5 * TOL_FP64, rel=1e-6)
        assert_matches_twin(got, twins)
        got[k][0] = _moved(twins[0][k], 2.0 * TOL_FP64)
        _refused(got, twins)
    got = _got(twins)
    got["P"][0] = _moved(got["P"][0], 2.0 * TOL_FP64)      # ... of the keys asked for
    assert_matches_twin(got, twins, keys="XF")
    _refused(got, twins, keys="XFP")


def test_a_nan_is_refused():
    twins = _twins()
    got = _got(twins)
    got["F"][1, 5] = np.nan
    _refused(got, twins)
    _refused(got, twins, spread_of=twins)


def test_the_bound_follows_the_spread_of_a_second_cpu_run():
    twins = _twins()
    spread = 1e-4
    for k in "XF":
        second = [dict(r) for r in twins]
        second[1][k] = _moved(twins[1][k], spread)
        for other in "XFP":
            got = _got(twins)
            got[other][1] = _moved(got[other][1], 0.5 * K_SPREAD * spread)
            assert_matches_twin(got, twins, spread_of=second)
            _refused(got, twins)                                        # (without the spread: 1e-5)
            got[other][1] = _moved(twins[1][other], 2.0 * K_SPREAD * spread)
            _refused(got, twins, spread_of=second)
            got[other][1], got[other][0] = twins[1][other], _moved(twins[0][other], 2.0 * TOL_FP64)      # no problem borrows another's spread
            _refused(got, twins, spread_of=second)


def test_left_out_problems_are_counted():
    twins = _twins()
    second = [dict(r) for r in twins]
    second[2]["stats"] = twins[2]["stats"] + np.array([0, 1, 0, 0, 0, 0])
    got = _got(twins)
    got["X"][2] = np.nan                                                # a problem left out is not compared
    assert assert_matches_twin(got, twins, disagree=second, may_skip=1) == 3
    _refused(got, twins, disagree=second)
    _refused(got, twins, may_skip=1)                                    # no second run, nothing left out
    second[0]["stats"] = twins[0]["stats"] + np.array([0, 0, 0, 1, 0, 0])
    _refused(got, twins, disagree=second, may_skip=1)
    assert assert_matches_twin(got, twins, disagree=second, may_skip=2) == 2
