"""The fp32 step decisions of the batch kernel (biconvex_lanes.h: seg_sum2_f32 / seg_sum1_f32, power-of-two segments; biconvex_admm_body.h:
BAND), restated in numpy: the segment sums in the exact order of the DPP / permlane butterflies, in float32 as
the kernels add them, against the exact sums; and the decisions taken from them when they are clear of their thresholds against
the decisions of the fp64 butterfly and the reference expression."""
import math

import numpy as np
import pytest

from tests.lanes_np import IS_P, _partner, _rows, _swap, desig, seg_sum, segments  # noqa: F401  (the restatements: tests/lanes_np.py)


def wide(rng, n):
    """non-negative terms over 40 decades, a few exact zeros"""
    x = rng.random(n) * 10.0 ** rng.uniform(-20, 20, n)
    x[rng.random(n) < 0.1] = 0.0
    return x


@pytest.mark.parametrize("lpp", [16, 32, 64])
def test_fp32_segment_sums_within_1e6(lpp):
    rng = np.random.default_rng(lpp)
    worst, n = 0.0, 0
    for trial in range(400):
        x = wide(rng, 64) if trial % 2 else rng.random(64) * 10.0 ** rng.uniform(-24, 24)
        if lpp == 21:
            x[63] = 0.0       # (lane 63 belongs to no segment)
        got = seg_sum(x.astype(np.float32), lpp)
        for d, seg in zip(desig(lpp), segments(lpp)):
            exact = math.fsum(x[seg])
            if not 1e-24 <= exact <= 1e30:
                continue
            worst = max(worst, abs(float(got[d]) - exact) / exact)
            n += 1
        if lpp != 21:      # every lane of a segment holds the same bits (LPP = 21: only the designated lanes are read)
            for seg in segments(lpp):
                assert np.all(got[seg].view(np.uint32) == got[seg[0]].view(np.uint32))
    assert n > 300 and worst < 1e-6, (n, worst)


def test_fp64_restatement_is_the_kernels_butterfly():
    """the same order in float64 is seg_sum2's: sums of integers are exact, and lanes of other segments never enter"""
    for lpp in (16, 21, 32, 64):
        x = np.arange(64, dtype=np.float64) + 1.0
        got = seg_sum(x, lpp)
        for d, seg in zip(desig(lpp), segments(lpp)):
            assert got[d] == x[seg].sum()


def fp64_decision(g2, cv, Lh, tol2, tol):
    """the fall-back: fp64 butterfly sums (given) and the reference expression with its sqrt band"""
    rhs = Lh * g2
    bt, done = cv > rhs, g2 < tol2
    if abs(cv - rhs) <= 1e-14 * rhs or abs(g2 - tol2) <= 1e-14 * tol2:
        gn = math.sqrt(g2)
        bt, done = cv > Lh * (gn * gn), gn < tol
    return bt, done


def band(x):
    return np.float32(x * (1.0 - 1e-5)), np.float32(x * (1.0 + 1e-5))


def fp32_decision(gf, cf, Lh, tol2):
    """the kernels' banded decision at one designated lane: (clear, retry, done)"""
    if 1e-3 <= Lh <= 1e30:
        llo, lhi = band(Lh)
    else:
        llo = lhi = np.float32("nan")
    t2lo, t2hi = band(tol2)
    with np.errstate(over="ignore", invalid="ignore"):
        yes, no = cf > gf * lhi, cf < gf * llo
        dyes, dno = gf < t2lo, gf > t2hi
        clear = (yes or no) and (dyes or dno) and np.float32(1e-24) <= gf <= np.float32(1e30)
    return bool(clear), bool(yes), bool(dyes)


@pytest.mark.parametrize("lpp", [16, 32, 64])
def test_band_clear_decisions_equal_fp64(lpp):
    rng = np.random.default_rng(100 + lpp)
    tol = 1e-5
    clear_n = total = 0
    for trial in range(600):
        g = wide(rng, 64) * 10.0 ** rng.uniform(-30, -8)
        if lpp == 21:
            g[63] = 0.0
        if trial % 3 == 0:      # g2 within a few 1e-5 of tol^2
            g *= tol * tol / max(seg_sum(g, lpp)[desig(lpp)[0]], 1e-300) * (1.0 + rng.normal(0, 3e-5))
        Lh = float(10.0 ** rng.uniform(-1, 7))
        s64g = seg_sum(g, lpp)
        f32g = seg_sum(g.astype(np.float32), lpp)
        w = np.abs(rng.normal(1.0, 0.3, 64))
        for d in desig(lpp):
            # cv within a few 1e-5 of the retry threshold (two trials of three), or anywhere
            scale = 1.0 + (rng.normal(0, 3e-5) if trial % 3 else rng.normal(0, 0.5))
            c = g * w
            sc = seg_sum(c, lpp)[d]
            if sc > 0:
                c = c * (Lh * s64g[d] / sc * scale)
            bt64, done64 = fp64_decision(float(s64g[d]), float(seg_sum(c, lpp)[d]), Lh, tol * tol, tol)
            clear, bt32, done32 = fp32_decision(f32g[d], seg_sum(c.astype(np.float32), lpp)[d], Lh, tol * tol)
            total += 1
            if clear:
                clear_n += 1
                assert (bt32, done32) == (bt64, done64), (lpp, trial, d)
    assert clear_n > total // 4, (clear_n, total)      # the shortcut is taken in many steps: the comparison is not vacuous


def test_nan_inf_and_out_of_range_sums_fall_back():
    f = np.float32
    for gf, cf in [(f("nan"), f(1)), (f(1), f("nan")), (f("inf"), f(1)), (f(1e-30), f(0)), (f(1e31), f(1))]:
        assert not fp32_decision(gf, cf, 250.0, 1e-10)[0], (gf, cf)
    assert not fp32_decision(f(1), f(1), 1e-4, 1e-10)[0]      # a step constant outside [1e-3, 1e30]
    assert fp32_decision(f(1e-3), f(1), 250.0, 1e-10) == (True, True, False)
    assert fp32_decision(f(1e-11), f(0), 250.0, 1e-10) == (True, False, True)
