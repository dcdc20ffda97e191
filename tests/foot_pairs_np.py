"""Numpy model of the headline kernel's force loop with two feet per lane ("Force loop: two feet per lane"): the
unit map of a 32-lane segment, and the six image sums as chains split over a knot's units.  A restatement in numpy of what
biconvex_admm_body.h does on the device, for tests/test_foot_pairs_cpu.py; every operation on float64, fma through math.fma where the
interpreter has it and through exact rational arithmetic where it does not."""
import fractions
import math

import numpy as np

LANES = 32


def contact_mask(an, sp):
    """bit n set: foot n is a contact foot.  an (E,), sp (E, 3) of one knot; a swing foot has an == 0 and all three sp == 0"""
    return sum(1 << n for n in range(len(an)) if not (an[n] == 0 and np.all(sp[n] == 0)))


def unit_map(masks):
    """The units of one problem, from its knots' contact masks (one per force knot, in knot order).  A list of (knot, rank, feet) with
    feet a tuple of at most two foot indices: knot t gets max(1, ceil(c_t / 2)) units, in knot order, a second unit directly behind the
    first, the contact feet in foot order."""
    units = []
    for t, m in enumerate(masks):
        feet = [n for n in range(4) if m >> n & 1]
        units.append((t, 0, tuple(feet[:2])))
        if len(feet) > 2:
            units.append((t, 1, tuple(feet[2:])))
    return units


def eligible(masks, F0):
    """at most 32 units, and every swing foot's three F0 values the bit pattern of +0.0.  F0 (H, E, 3)"""
    if len(unit_map(masks)) > LANES:
        return False
    F0 = np.asarray(F0, np.float64)
    for t, m in enumerate(masks):
        for n in range(F0.shape[1]):
            if not m >> n & 1 and np.any(F0[t, n].view(np.uint64) != 0):
                return False
    return True


def fma(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    exact = fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c)
    if exact == 0:      # the sign of an exact zero: that of the sum of the (signed zero) product and c under round-to-nearest
        return a * b + c if a * b == 0 else 0.0
    return float(exact)


def cross_terms(sp, v):
    """the three cross products of one foot as the kernel makes them, once: fma(sp2, vy, -(sp1 vz)) and its two rotations"""
    return (fma(sp[2], v[1], -(sp[1] * v[2])), fma(sp[0], v[2], -(sp[2] * v[0])), fma(sp[1], v[0], -(sp[0] * v[1])))


def chain(s, an, sp, v):
    """one foot's link of the six image sums, on s (6,): the first three by fma, the last three by adding the foot's cross terms"""
    u = cross_terms(sp, v)
    return [fma(an, v[k], s[k]) for k in range(3)] + [np.float64(s[3 + k]) + np.float64(u[k]) for k in range(3)]


def image_four_feet(an, sp, v):
    """the four-foot loop's sums of one knot: the chain over feet 0..3 from +0.  an (4,), sp (4, 3), v (4, 3)"""
    s = [0.0] * 6
    for n in range(4):
        s = chain(s, an[n], sp[n], v[n])
    return np.array(s, np.float64)


def image_units(mask, an, sp, v, swap=False):
    """... and the two-feet-per-lane loop's: the first unit's chain from +0 over its slots, continued by the second unit's (swap: the
    second unit first -- the order that must NOT give the four-foot bits)"""
    units = unit_map([mask])
    if swap:
        units = units[::-1]
    s = [0.0] * 6
    for _, _, feet in units:
        for n in feet:
            s = chain(s, an[n], sp[n], v[n])
    return np.array(s, np.float64)
