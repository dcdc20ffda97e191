"""The force loop with two feet per lane ("Force loop: two feet per lane"), on the CPU: the unit map of a segment and
the split chains of the image sums, through the numpy model tests/foot_pairs_np.py.

The signed-zero statement of the design is checked here and not assumed: dropping a swing foot's links (fma(0, +0, s) and s + (+0)) can
change a sum only from -0 to +0, and a chain that starts from +0 never holds -0 -- fma(a, b, s) and s + u are -0 under round-to-nearest
only if s is -0 too.  So the sums of the two loops are equal bit for bit in every case below, the ones with -0.0 slot values included,
and the tests assert exactly that: no case differs in a zero's sign."""
import itertools

import numpy as np
import pytest

from bunmpc_amd import problems
from tests import foot_pairs_np as fp


def _check_map(masks):
    units = fp.unit_map(masks)
    knots = [u[0] for u in units]
    assert knots == sorted(knots) and sorted(set(knots)) == list(range(len(masks)))      # knot order, every knot present
    for i, (t, rank, feet) in enumerate(units):
        assert len(feet) <= 2 and list(feet) == sorted(feet)
        if rank == 1:
            assert i > 0 and units[i - 1][0] == t and units[i - 1][1] == 0      # directly behind its first unit
            assert len(units[i - 1][2]) == 2 and len(feet) >= 1
        else:
            assert i == 0 or units[i - 1][0] == t - 1
    for t, m in enumerate(masks):
        placed = [n for u in units if u[0] == t for n in u[2]]
        assert placed == [n for n in range(4) if m >> n & 1]      # every contact foot exactly once, in foot order
        assert sum(1 for u in units if u[0] == t) == max(1, -(-bin(m).count("1") // 2))
    return units


@pytest.mark.parametrize("H", [16, 17, 18, 19, 20])
def test_unit_map_of_every_contact_count(H):
    """17 .. 21 knots, every contact count 0 .. 4 somewhere in the plan, every set of feet"""
    masks = [(5 * t + 3) % 16 for t in range(H)]
    assert {bin(m).count("1") for m in masks} == {0, 1, 2, 3, 4}
    units = _check_map(masks)
    assert len(units) == H + sum(bin(m).count("1") > 2 for m in masks)


def _masks_of(b, i):
    an = b.cnt_plan[i, :, :, 0] * (b.dt[i][:, None] / b.m)
    sp = b.cnt_plan[i, :, :, :1] * (b.x_init[i, None, None, :3] - b.cnt_plan[i, :, :, 1:]) * b.dt[i][:, None, None]
    return [fp.contact_mask(an[t], sp[t]) for t in range(b.H)]


def test_the_trot_plan_takes_28_units():
    """the benchmark's batch: 12 knots with two feet in the air, 8 in full stance -- 12 + 2 x 8 lanes"""
    b = problems.make_batch("solo12_trot", 6, H=20)
    for i in range(b.B):
        masks = _masks_of(b, i)
        assert sorted(bin(m).count("1") for m in masks) == [2] * 12 + [4] * 8
        assert len(_check_map(masks)) == 28
        assert fp.eligible(masks, np.zeros((20, 4, 3)))


def test_the_mixed_plans_take_26_to_28_units():
    b = problems.make_batch("solo12_mixed", 24, H=20)
    counts = set()
    for i in range(b.B):
        masks = _masks_of(b, i)
        counts.add(len(_check_map(masks)))
        assert fp.eligible(masks, np.zeros((20, 4, 3)))
    assert counts <= {26, 27, 28} and {26, 28} <= counts, counts


def test_an_all_stance_plan_is_not_eligible():
    masks = [15] * 20
    assert len(_check_map(masks)) == 40
    assert not fp.eligible(masks, np.zeros((20, 4, 3)))


def test_a_swing_force_that_is_not_plus_zero_is_not_eligible():
    masks = [5] * 20
    F0 = np.zeros((20, 4, 3))
    assert fp.eligible(masks, F0)
    F0[7, 1, 2] = -0.0
    assert not fp.eligible(masks, F0)
    F0[7, 1, 2] = 0.0
    F0[7, 0, 2] = 3.0      # (a contact foot's force is free)
    assert fp.eligible(masks, F0)
    F0[3, 3, 0] = 1e-300
    assert not fp.eligible(masks, F0)


def test_random_plans():
    rng = np.random.default_rng(7)
    for _ in range(200):
        H = int(rng.integers(16, 21))
        masks = [int(m) for m in rng.integers(0, 16, H)]
        units = _check_map(masks)
        assert fp.eligible(masks, np.zeros((H, 4, 3))) == (len(units) <= 32)


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


FEET = [(0, 3), (1, 2), (0, 1, 2), (0, 1, 2, 3), (2,), ()]


@pytest.mark.parametrize("feet", FEET)
def test_split_chains_have_the_four_foot_bits(feet):
    """random operands, then operands made of signed zeros and of values that cancel exactly: the chain over the contact feet alone, split
    over the knot's units, against the chain over all four feet with the swing feet's exact zeros.  Equal by value (np.array_equal) --
    and, counted here, in no case different in a zero's sign."""
    rng = np.random.default_rng(11 + sum(1 << n for n in feet))
    mask = sum(1 << n for n in feet)
    sign_differences = 0
    for trial in range(300):
        an, sp, v = np.zeros(4), np.zeros((4, 3)), np.zeros((4, 3))
        for n in feet:
            an[n] = rng.uniform(0.001, 0.01)
            sp[n] = rng.normal(size=3) * 0.01
            v[n] = rng.normal(size=3) * 10.0
        if trial % 3 == 1:      # slots with -0.0 and +0.0 values, and feet whose products are zeros of either sign
            for n in feet:
                v[n] = rng.choice([-0.0, 0.0, 1.5, -2.5], size=3)
                sp[n] = rng.choice([-0.0, 0.0, 0.25, -0.5], size=3)
        if trial % 3 == 2 and len(feet) >= 2:      # sums that cancel exactly
            a, b = feet[0], feet[-1]
            an[b], sp[b], v[b] = an[a], sp[a], -v[a]
        assert fp.contact_mask(an, sp) == mask      # (an != 0 on every contact foot, whatever sp drew)
        four = fp.image_four_feet(an, sp, v)
        two = fp.image_units(mask, an, sp, v)
        assert np.array_equal(four, two), (feet, trial)
        sign_differences += int(np.sum(_bits(four) != _bits(two)))
    assert sign_differences == 0


def test_the_order_of_the_units_matters():
    """the sensitivity of the test above: with the knot's two units swapped in the chain some sum has other bits"""
    rng = np.random.default_rng(5)
    differing = 0
    for _ in range(100):
        an, sp, v = rng.uniform(0.001, 0.01, 4), rng.normal(size=(4, 3)) * 0.01, rng.normal(size=(4, 3)) * 10.0
        differing += not np.array_equal(fp.image_four_feet(an, sp, v), fp.image_units(15, an, sp, v, swap=True))
    assert differing > 50


def test_every_pair_and_triple_of_feet():
    rng = np.random.default_rng(3)
    for k in (2, 3):
        for feet in itertools.combinations(range(4), k):
            an, sp, v = np.zeros(4), np.zeros((4, 3)), np.zeros((4, 3))
            for n in feet:
                an[n], sp[n], v[n] = rng.uniform(0.001, 0.01), rng.normal(size=3) * 0.01, rng.normal(size=3) * 10.0
            mask = sum(1 << n for n in feet)
            assert np.array_equal(_bits(fp.image_four_feet(an, sp, v)), _bits(fp.image_units(mask, an, sp, v)))
