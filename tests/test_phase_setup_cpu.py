"""The statement the headline kernel's once-per-solve unit map rests on ("Force loop: two feet per lane"): the map of
a problem is a function of its contact plan alone.  The kernel builds it in front of the ADMM loop from the feet whose an = c (dt / m) is
not zero; a force phase used to build it from the phase's own an and sp = c (X - r) dt, X being the iterate of that phase.  Restated in
numpy with the model of tests/foot_pairs_np.py: over random plans and 17 .. 21 knots both rules name the same contact feet whatever
finite X the phase holds, so the same units, the same first lanes and the same `fits`; and where they do not -- a non-finite X -- the
phase's own test (a foot with an == 0 whose sp is not zero) says so, which sends the wave to four feet per lane."""
import numpy as np
import pytest

from tests import foot_pairs_np as fp

M = 2.5


def _plan(rng, H):
    """flags (H, 4) with every contact count present, positions r (H, 4, 3), dt (H,)"""
    c = (rng.random((H, 4)) < rng.choice([0.3, 0.5, 0.7])).astype(np.float64)
    c[rng.integers(H)] = 0.0
    c[rng.integers(H)] = [1.0, 1.0, 1.0, 0.0]
    return c, rng.normal(size=(H, 4, 3)), rng.choice([0.03, 0.05, 0.08], size=H)


def _phase_masks(c, r, dt, X):
    """the contact masks as a force phase sees them: the prologue's an and sp, on the phase's X (H, 3)"""
    an = c * (dt / M)[:, None]
    sp = c[:, :, None] * (X[:, None, :] - r) * dt[:, None, None]
    return [fp.contact_mask(an[t], sp[t]) for t in range(len(c))], an, sp


def _plan_masks(c, dt):
    """... and as the kernel takes them from the plan, once per solve"""
    return [sum(1 << n for n in range(4) if c[t, n] * (dt[t] / M) != 0) for t in range(len(c))]


def _starts(masks):
    """the kernel's scatter: knot t's first unit sits on lane t + (knots in front of it that take two units); its mask of such knots"""
    two = sum(1 << t for t, m in enumerate(masks) if bin(m).count("1") > 2)
    return [t + bin(two & ((1 << t) - 1)).count("1") for t in range(len(masks))], two


def _stale(an, sp):
    """the phase's test of the plan's map: some foot without contact in the plan whose sp is not zero in this phase"""
    return any(an[t, n] == 0 and not np.all(sp[t, n] == 0) for t in range(an.shape[0]) for n in range(an.shape[1]))


@pytest.mark.parametrize("H", [16, 17, 18, 19, 20])
def test_the_map_is_a_function_of_the_plan(H):
    rng = np.random.default_rng(100 + H)
    for _ in range(40):
        c, r, dt = _plan(rng, H)
        plan = _plan_masks(c, dt)
        units = fp.unit_map(plan)
        starts, two = _starts(plan)
        assert [i for i, u in enumerate(units) if u[1] == 0] == starts
        assert len(units) == H + bin(two).count("1")
        for scale in (0.0, 1.0, 1e-300, 1e150):      # ten phases' worth of iterates, tiny and huge ones among them
            for _ in range(3):
                X = scale * rng.normal(size=(H, 3))
                t = int(rng.integers(H))
                X[t] = r[t, rng.integers(4)]      # (a foot exactly under the centre of mass: sp = 0, an != 0)
                masks, an, sp = _phase_masks(c, r, dt, X)
                assert masks == plan
                assert not _stale(an, sp)
                assert fp.unit_map(masks) == units and _starts(masks) == (starts, two)


def test_a_contact_foot_with_zero_dt_is_no_contact_under_both_rules():
    rng = np.random.default_rng(7)
    c, r, dt = _plan(rng, 20)
    c[3] = 1.0
    dt[3] = 0.0
    masks, an, sp = _phase_masks(c, r, dt, rng.normal(size=(20, 3)))
    assert masks[3] == 0 and masks == _plan_masks(c, dt) and not _stale(an, sp)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_iterate_is_seen_by_the_phase(bad):
    """0 (X - r) dt is NaN for a non-finite X: the phase's rule takes the swing foot for a contact foot, the plan's does not; the phase's
    test fires exactly where the two differ"""
    rng = np.random.default_rng(11)
    for _ in range(50):
        H = int(rng.integers(16, 21))
        c, r, dt = _plan(rng, H)
        X = rng.normal(size=(H, 3))
        t = int(rng.integers(H))
        X[t, rng.integers(3)] = bad
        with np.errstate(invalid="ignore"):
            masks, an, sp = _phase_masks(c, r, dt, X)
        differs = masks != _plan_masks(c, dt)
        assert differs == bool(np.any(c[t] == 0))
        assert _stale(an, sp) == differs
