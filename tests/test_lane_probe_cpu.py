"""bmpc_probe_lanes (include/bunmpc.h) refuses bad arguments before any device call, and the lane models of tests/lanes_np.py, which
test_lane_probe_gpu.py holds the device to, agree with each other and with exact arithmetic.  No GPU."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from bunmpc_amd import _lib
from tests import lanes_np as ln
from tests.test_lane_screen_cpu import _partials
from tests.test_step_decisions_cpu import wide

GROUPS = {name[len("BMPC_PROBE_"):]: v for name, v in _lib._ABI.defines.items() if name.startswith("BMPC_PROBE_")}
ROWS = {"SUM64": (2, 16), "SUM32": (2, 9), "SHIFT": (2, 4), "MASK": (2, 9), "THETA": (2, 1), "ARITH": (7, 17), "BANDED": (4, 3)}      # (in, out) rows of 64 words per wave


def test_the_groups_are_the_headers():
    assert sorted(GROUPS.values()) == list(range(7)) and set(GROUPS) == set(ROWS)


def test_bad_arguments_are_refused_without_a_device(hiplib):
    buf = (C.c_ulonglong * (64 * 17 * 2))()
    for name, (nin, nout) in ROWS.items():
        g, wi, wo = GROUPS[name], 512 * nin, 512 * nout
        bad = [(g, None, wi, buf, wo), (g, buf, wi, None, wo),                     # a null pointer
               (g, buf, 0, buf, 0), (g, buf, -wi, buf, -wo),                       # no wave
               (g, buf, wi + 8, buf, wo), (g, buf, wi - 8, buf, wo), (g, buf, wi + 256, buf, wo),      # not a whole number of waves
               (g, buf, wi, buf, wo + 8), (g, buf, wi, buf, wo - 8), (g, buf, 2 * wi, buf, wo), (g, buf, wi, buf, 2 * wo),      # out does not fit in
               (g, buf, ((1 << 20) + 1) * wi, buf, ((1 << 20) + 1) * wo)]          # more waves than a call takes
        for args in bad:
            assert hiplib.bmpc_probe_lanes(*args) == _lib.BAD_ARG, (name, args[2], args[4])
            assert hiplib.bmpc_last_error()
    for g in (-1, 7, 1 << 20):
        assert hiplib.bmpc_probe_lanes(g, buf, 1024, buf, 1024) == _lib.BAD_ARG
        assert b"group" in hiplib.bmpc_last_error()


def test_seg_sum_32_is_butterfly_sum32_bit_for_bit():
    """the two restatements of seg_sum<32> -- on a wave of 64 lanes (the step decisions' proofs) and on [..., 32] partials (the screen's) --
    on the screen test's partials: zero, denormal, inf and NaN lanes included"""
    p, _ = _partials(np.random.default_rng(20), 4000)
    want = ln.butterfly_sum32(p)
    nans = 0
    for r in range(0, len(p), 2):
        got = ln.seg_sum(np.concatenate([p[r], p[r + 1]]), 32)
        for half in (0, 1):
            seg, w = got[32 * half:32 * half + 32], want[r + half]
            if np.isnan(w):
                nans += 1
                assert np.all(np.isnan(seg))
            else:
                assert np.all(seg.view(np.uint64) == w.view(np.uint64))
    assert nans > 10


def test_round_fraction_is_correct_rounding():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(300) * 10.0 ** rng.uniform(-150, 150, 300)
    b = rng.standard_normal(300) * 10.0 ** rng.uniform(-150, 150, 300)
    for x, y in zip(a, b):
        q = Fraction(x) / Fraction(y)
        assert ln.round_fraction(q) == float(q) and ln.fast_div(np.float64(x), np.float64(y)) == x / y      # (int / int and IEEE division round correctly)
        assert ln.fma(np.float64(x), np.float64(1.0), np.float64(y)) == x + y and ln.fma(np.float64(x), np.float64(y), np.float64(0.0)) == x * y
    # ties to even, the subnormal range, float32
    assert ln.round_fraction(Fraction(2 ** 53 + 1)) == 2.0 ** 53 and ln.round_fraction(Fraction(2 ** 53 + 3)) == 2.0 ** 53 + 4
    assert ln.round_fraction(Fraction(3, 2 ** 1075)) == 2 * 5e-324 and ln.round_fraction(Fraction(1, 2 ** 1075)) == 0.0
    assert ln.round_fraction(-Fraction(5, 2 ** 1075)) == -2 * 5e-324
    f = ln.round_fraction(Fraction(2 ** 24 + 1), np.float32)
    assert type(f) is np.float32 and f == np.float32(2 ** 24)
    fa, fb = rng.standard_normal(300).astype(np.float32), rng.standard_normal(300).astype(np.float32)
    for x, y in zip(fa, fb):
        assert ln.fast_div(x, y) == x / y and type(ln.fast_div(x, y)) is np.float32
    # fma rounds once: 1 + 2^-53 + 2^-106 is above the tie that the product rounded first would fall on
    e = np.float64(2.0 ** -53)
    assert ln.fma(e, e, np.float64(1.0) + 2 * e) == 1.0 + 2 * e and ln.fma(np.float64(1.0) + 2 * e, np.float64(1.0) + 2 * e, -np.float64(1.0)) == 4 * e + 4 * e * e
    z = ln.fma(np.float64(-0.0), np.float64(1.0), np.float64(-0.0))
    assert z == 0.0 and np.signbit(z) and not np.signbit(ln.fma(np.float64(1.0), np.float64(1.0), np.float64(-1.0)))


def test_masks_against_a_lane_by_lane_count():
    rng = np.random.default_rng(9)
    for _ in range(500):
        have, need = (ln.mask_of(rng.choice(64, int(rng.integers(0, 6)), replace=False)) for _ in range(2))      # (sparse: segments without a bit)
        h, n = ln.lanes(have), ln.lanes(need)
        assert ln.mask_of(np.flatnonzero(h)) == have
        for lpp in (16, 32, 64):
            assert ln.seg_covered(have, need, lpp) == all(h[s].any() or not n[s].any() for s in ln.segments(lpp))
        assert ln.seg_covered32(have, *ln.seg_dead32(need)) == ln.seg_covered(have, need, 32)
        d = ln.lanes(ln.seg_uniform(have & ln.seg_desig(21), 21))
        for k, s in enumerate(ln.segments(21)):
            assert np.all(d[s] == h[16 * (k + 1)])
        assert not d[63]


def test_the_order_of_additions_shows_in_random_sums():
    """what makes bit equality with the model a test: the butterflies differ from a left-to-right sum, and a 21-lane segment's sum from
    the same terms in another segment (splits 16|5, 11|10, 6|15), in a good share of random draws -- all within gamma_6 of the exact sum"""
    rng = np.random.default_rng(5)
    u = 2.0 ** -53
    gamma = 6 * u / (1 - 6 * u)
    n = 400
    differs = {lpp: 0 for lpp in (16, 21, 32, 64)}
    moved = 0
    for _ in range(n):
        x = wide(rng, 64)
        for lpp in differs:
            s = ln.seg_sum(x, lpp)
            differs[lpp] += any(s[d] != np.add.reduce(x[seg]) for d, seg in zip(ln.desig(lpp), ln.segments(lpp)))
        t = wide(rng, 21)
        sums = []
        for k in range(3):
            v = np.zeros(64)
            v[21 * k:21 * k + 21] = t
            sums.append(float(ln.seg_sum(v, 21)[16 * (k + 1)]))
        exact = math.fsum(t)
        assert all(abs(s - exact) <= gamma * exact for s in sums)
        moved += len(set(sums)) > 1
    print("cases that differ from a left-to-right sum", differs, "| 21 terms whose sum depends on the segment: %d of %d" % (moved, n))
    assert all(v > n // 10 for v in differs.values()) and moved > n // 10


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_shifts_and_keep_if_move_bits(dtype):
    ut = np.uint64 if dtype is np.float64 else np.uint32
    v = np.arange(1, 65).astype(ut).view(dtype)      # (subnormals: only the bits matter)
    v[5] = np.array([0x7ff4000000000123 if dtype is np.float64 else 0x7fa00123], ut).view(dtype)[0]      # a signalling NaN with a payload
    assert np.all(ln.from_prev(v).view(ut)[1:] == v.view(ut)[:-1]) and ln.from_prev(v).view(ut)[0] == 0
    assert np.all(ln.from_next(v).view(ut)[:-1] == v.view(ut)[1:]) and ln.from_next(v).view(ut)[63] == 0
    m = np.where(np.arange(64) % 2 == 0, -1, 0)
    k = ln.keep_if(v, m)
    assert np.all(k.view(ut)[::2] == v.view(ut)[::2]) and np.all(k.view(ut)[1::2] == 0)
