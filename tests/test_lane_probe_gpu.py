"""The lane helpers of the centroidal kernels (bunmpc_amd/csrc/biconvex_lanes.h) on the device, through bmpc_probe_lanes, against their
models (tests/lanes_np.py): bit for bit, at every LPP a kernel instantiates them with.  A wave is a test case, a group is one launch.
The models are what the CPU proofs argue about (test_step_decisions_cpu.py, test_lane_screen_cpu.py, test_term_screen_cpu.py); the
order of additions, the P / Q parts of a 21-lane segment, the zeros at the wave's ends and the isolation of a segment's NaN are pinned
here.  gamma = 6u / (1 - 6u), u = 2^-53, bounds the relative error of a sum of non-negative terms in which no term passes through more
than six additions: four row stages and at most two swaps, or four stages and the add of the two parts of a 21-lane segment."""
import math
from fractions import Fraction

import numpy as np
import pytest

from bunmpc_amd import _lib
from tests import lanes_np as ln
from tests.test_lane_probe_cpu import GROUPS, ROWS
from tests.test_lane_screen_cpu import _partials, _thresholds
from tests.test_step_decisions_cpu import wide

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GAMMA = 6 * U / (1 - 6 * U)
LPPS = (16, 21, 32, 64)
U64, U32 = np.uint64, np.uint32


def probe(hiplib, group, rows):
    """rows: [waves][NIN][64] uint64 -> [waves][NOUT][64] uint64"""
    nin, nout = ROWS[group]
    rows = np.ascontiguousarray(rows, U64)
    assert rows.ndim == 3 and rows.shape[1:] == (nin, 64)
    out = np.full((rows.shape[0], nout, 64), 0xdeadbeefdeadbeef, U64)
    _lib.check(hiplib.bmpc_probe_lanes(GROUPS[group], rows.ctypes.data, rows.nbytes, out.ctypes.data, out.nbytes))
    return out


def w64(x):
    return np.ascontiguousarray(x, np.float64).view(U64)


def w32(x):
    return np.ascontiguousarray(x, np.float32).view(U32).astype(U64)


def f64(w):
    return np.ascontiguousarray(w).view(np.float64)


def f32(w):
    return np.ascontiguousarray(w).astype(U32).view(np.float32)


def same_bits(a, b):
    ut = U64 if a.dtype == np.float64 else U32
    return np.ascontiguousarray(a).view(ut) == np.ascontiguousarray(b).view(ut)


def sum_inputs(rng, n, dtype):
    """{kind: [n][64]}: non-negative terms over 40 decades; mixed signs with cancellation; subnormals (and the smallest normals beside
    them); signed zeros with a few ordinary terms"""
    tiny, mant = (5e-324, 2 ** 52) if dtype is np.float64 else (float(np.float32(1e-45)), 2 ** 23)
    x = np.stack([wide(rng, 64) for _ in range(n)])
    mixed = rng.standard_normal((n, 64)) * 10.0 ** rng.uniform(-3, 3, (n, 64))
    mixed[:, 1::2] = np.where(rng.random((n, 32)) < 0.7, -mixed[:, 0::2] * (1.0 + rng.integers(-4, 5, (n, 32)) * 2.0 ** -50), mixed[:, 1::2])
    mixed = rng.permuted(mixed, axis=1)
    sub = rng.integers(0, mant, (n, 64)).astype(np.float64) * tiny * rng.choice([1.0, 1.0, 4.0, 2048.0], (n, 64)) * rng.choice([1.0, -1.0], (n, 64))
    zeros = np.where(rng.random((n, 64)) < 0.5, 0.0, -0.0)
    zeros[: n // 2] = np.where(rng.random((n // 2, 64)) < 0.1, rng.standard_normal((n // 2, 64)), zeros[: n // 2])
    zeros[-1] = -0.0
    zeros[-2] = 0.0
    with np.errstate(over="ignore", under="ignore"):
        return {k: v.astype(dtype) for k, v in (("wide", x), ("mixed", mixed), ("subnormal", sub), ("zeros", zeros))}


@pytest.fixture(scope="module")
def sums64(hiplib):
    """one launch: 4 kinds x 500 waves, a and b different draws"""
    rng = np.random.default_rng(64)
    a, b = sum_inputs(rng, 500, np.float64), sum_inputs(rng, 500, np.float64)
    kinds = list(a)
    A, B = np.concatenate([a[k] for k in kinds]), np.concatenate([b[k] for k in kinds])
    out = f64(probe(hiplib, "SUM64", np.stack([w64(A), w64(B)], axis=1)))
    return kinds, A, B, out


def valid_lanes(lpp, which):
    """which: 0 seg_sum (every lane of the segments), 1..3 seg_sum2 / seg_sum1 (LPP = 21: the designated lanes)"""
    if lpp != 21:
        return np.arange(64)
    return np.arange(63) if which == 0 else ln.desig(21)


def test_fp64_segment_sums_have_the_models_bits(sums64):
    kinds, A, B, out = sums64
    n = len(A) // len(kinds)
    for i, lpp in enumerate(LPPS):
        want = [ln.seg_sum_all(A, lpp), ln.seg_sum(A, lpp), ln.seg_sum(B, lpp), ln.seg_sum(A, lpp)]
        for which in range(4):
            v = valid_lanes(lpp, which)
            ok = same_bits(out[:, 4 * i + which][:, v], want[which][:, v])
            for k, kind in enumerate(kinds):
                assert ok[k * n:(k + 1) * n].all(), (lpp, which, kind, int((~ok[k * n:(k + 1) * n]).sum()))
        d = ln.desig(lpp)
        # seg_sum2's first result is seg_sum1's, and seg_sum's where both are valid
        assert same_bits(out[:, 4 * i + 1][:, d], out[:, 4 * i + 3][:, d]).all() and same_bits(out[:, 4 * i + 1][:, d], out[:, 4 * i][:, d]).all()
        if lpp != 21:      # every lane of a segment holds the same bits
            for which in range(4):
                for seg in ln.segments(lpp):
                    assert same_bits(out[:, 4 * i + which][:, seg], out[:, 4 * i + which][:, seg[:1]]).all(), (lpp, which)
        else:
            for k, seg in enumerate(ln.segments(21)):
                assert same_bits(out[:, 4][:, seg], out[:, 4][:, 16 * (k + 1)][:, None]).all()


def test_fp64_sums_see_the_order_and_stay_within_gamma(sums64):
    kinds, A, B, out = sums64
    n = len(A) // len(kinds)
    x, got = A[:n], out[:n]      # the non-negative kind
    assert kinds[0] == "wide" and np.all(x >= 0)
    for i, lpp in enumerate(LPPS):
        differs, worst = 0, 0.0
        for d, seg in zip(ln.desig(lpp), ln.segments(lpp)):
            differs += int((~same_bits(got[:, 4 * i + 1, d], np.add.reduce(x[:, seg], axis=1))).sum())
            for w in range(n):
                exact = math.fsum(x[w, seg])
                if exact > 0:
                    worst = max(worst, abs(Fraction(float(got[w, 4 * i + 1, d])) - Fraction(exact)) / Fraction(exact))
        print("LPP %d: %d segment sums differ from np.add.reduce; largest error %.2f u" % (lpp, differs, float(worst) / U))
        assert differs > 0
        assert worst <= GAMMA


def poisoned(rng, lpp, dtype):
    """[(zeroed wave pair, poisoned wave pair, lanes whose sums must not move)]: one segment of a and b filled with NaN / +inf / -inf (all of
    one kind, or mixed with ordinary terms), at every position of the segment"""
    cases = []
    for k, seg in enumerate(ln.segments(lpp)):
        others = np.setdiff1d(np.concatenate(ln.segments(lpp)), seg)
        for fill in (np.nan, np.inf, -np.inf, "mixed"):
            a, b = wide(rng, 64).astype(dtype), wide(rng, 64).astype(dtype)
            za, zb, pa, pb = a.copy(), b.copy(), a.copy(), b.copy()
            za[seg] = zb[seg] = 0
            bad = rng.choice([np.nan, np.inf, -np.inf, 1.0], len(seg)) if fill == "mixed" else np.full(len(seg), fill)
            bad[0] = np.nan if fill == "mixed" else bad[0]
            pa[seg] = pb[seg] = bad.astype(dtype)
            cases.append(((za, zb), (pa, pb), others))
    return cases


def test_fp64_nan_and_inf_stay_in_their_segment(hiplib):
    rng = np.random.default_rng(7)
    cases = [(lpp, c) for lpp in (16, 21, 32) for c in poisoned(rng, lpp, np.float64)]
    a = wide(rng, 64)
    nan63 = a.copy()
    nan63[63] = np.nan
    zero63 = a.copy()
    zero63[63] = 0.0
    cases.append((21, ((zero63, zero63), (nan63, nan63), np.arange(63))))      # lane 63 belongs to no segment (the self test zeroes it)
    rows = np.stack([np.stack([w64(p[0]), w64(p[1])]) for _, c in cases for p in c[:2]])
    out = f64(probe(hiplib, "SUM64", rows))
    for j, (lpp, (_, _, others)) in enumerate(cases):
        i = LPPS.index(lpp)
        zeroed, bad = out[2 * j], out[2 * j + 1]
        for which in range(4):
            v = np.intersect1d(valid_lanes(lpp, which), others)
            assert len(v) and np.all(np.isfinite(zeroed[4 * i + which][v]))
            assert same_bits(zeroed[4 * i + which][v], bad[4 * i + which][v]).all(), (lpp, j, which)
        if len(others) < 63:      # ... and the segment's own sum is not finite
            own = np.setdiff1d(np.arange(63 if lpp == 21 else 64), others)
            assert not np.isfinite(bad[4 * i][own]).any()
    # one segment only at LPP = 64: a NaN lane makes the wave's sum NaN
    assert np.isnan(out[1][12]).all()


def test_a_21_lane_sum_depends_on_its_segment_within_2_gamma(hiplib):
    """the same 21 non-negative terms in segment 0, 1 and 2 (splits 16|5, 11|10, 6|15 over the DPP rows): each sum has the model's bits for
    its position, the three are within 2 gamma of the exact sum of each other, and they DO differ in a good share of the cases"""
    rng = np.random.default_rng(21)
    n = 600
    t = np.stack([wide(rng, 21) for _ in range(n)])
    waves = np.stack([wide(rng, 64) for _ in range(3 * n)]).reshape(n, 3, 64)      # (the rest of the wave: other problems' terms)
    for k in range(3):
        waves[:, k, 21 * k:21 * k + 21] = t
    flat = waves.reshape(3 * n, 64)
    out = f64(probe(hiplib, "SUM64", np.stack([w64(flat), w64(flat[::-1])], axis=1))).reshape(n, 3, 16, 64)
    model = ln.seg_sum(flat, 21).reshape(n, 3, 64)
    sums = np.stack([out[:, k, 5, 16 * (k + 1)] for k in range(3)], axis=1)
    assert same_bits(sums, np.stack([model[:, k, 16 * (k + 1)] for k in range(3)], axis=1)).all()
    assert same_bits(sums, np.stack([out[:, k, 4, 21 * k] for k in range(3)], axis=1)).all()      # seg_sum<21>, any lane of the segment
    moved = 0
    for w in range(n):
        exact = math.fsum(t[w])
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert abs(Fraction(float(sums[w, i])) - Fraction(float(sums[w, j]))) <= Fraction(2 * GAMMA) * Fraction(exact), (w, i, j)
        moved += len(set(sums[w].tolist())) > 1
    print("21 terms moved between the segments: %d of %d sums differ (%.1f %%)" % (moved, n, 100.0 * moved / n))
    assert moved > n // 10


def test_fp32_segment_sums_have_the_models_bits(hiplib):
    rng = np.random.default_rng(32)
    a, b = sum_inputs(rng, 400, np.float32), sum_inputs(rng, 400, np.float32)
    kinds = list(a)
    A, B = np.concatenate([a[k] for k in kinds]), np.concatenate([b[k] for k in kinds])
    cases = [(lpp, c) for lpp in (16, 32) for c in poisoned(rng, lpp, np.float32)]
    PA = np.stack([p[0] for _, c in cases for p in c[:2]])
    PB = np.stack([p[1] for _, c in cases for p in c[:2]])
    out = f32(probe(hiplib, "SUM32", np.stack([w32(np.concatenate([A, PA])), w32(np.concatenate([B, PB]))], axis=1)))
    got, bad = out[:len(A)], out[len(A):]
    differs = {}
    for i, lpp in enumerate((16, 32, 64)):
        want = [ln.seg_sum(A, lpp), ln.seg_sum(B, lpp), ln.seg_sum(A, lpp)]
        for which in range(3):
            ok = same_bits(got[:, 3 * i + which], want[which])
            assert ok.all(), (lpp, which, [kinds[k] for k in np.unique(np.flatnonzero(~ok.all(axis=1)) // 400)])
            for seg in ln.segments(lpp):      # every lane of a segment holds the same bits
                assert same_bits(got[:, 3 * i + which][:, seg], got[:, 3 * i + which][:, seg[:1]]).all()
        differs[lpp] = int(sum((~same_bits(got[:400, 3 * i, seg[0]], np.add.reduce(A[:400][:, seg], axis=1, dtype=np.float32))).sum() for seg in ln.segments(lpp)))
    print("fp32 segment sums that differ from np.add.reduce:", differs)
    assert all(v > 0 for v in differs.values())
    for j, (lpp, (_, _, others)) in enumerate(cases):      # a segment's NaN / inf stays its own
        i = (16, 32, 64).index(lpp)
        for which in range(3):
            assert np.all(np.isfinite(bad[2 * j][3 * i + which][others]))
            assert same_bits(bad[2 * j][3 * i + which][others], bad[2 * j + 1][3 * i + which][others]).all(), (lpp, j, which)
            own = np.setdiff1d(np.arange(64), others)
            assert not np.isfinite(bad[2 * j + 1][3 * i + which][own]).any()


def test_shifts_move_bits_and_read_zero_at_the_wave_ends(hiplib):
    rng = np.random.default_rng(1)
    n = 300
    d = rng.integers(0, 1 << 64, (n, 64), dtype=U64)      # every bit pattern: NaN payloads (signalling ones too), infinities, subnormals
    f = rng.integers(0, 1 << 32, (n, 64), dtype=U64)
    d[0], f[0] = w64(np.full(64, -0.0)), w32(np.full(64, -0.0))
    d[1, ::2], f[1, ::2] = 0x7ff0000000000001, 0x7f800001
    d[2], f[2] = 0xfff8000000000abc, 0xffc00abc
    out = probe(hiplib, "SHIFT", np.stack([d, f], axis=1))
    assert np.array_equal(out[:, 0], ln.from_prev(d)) and np.array_equal(out[:, 1], ln.from_next(d))
    assert np.array_equal(out[:, 2], ln.from_prev(f)) and np.array_equal(out[:, 3], ln.from_next(f))
    assert not out[:, 0, 0].any() and not out[:, 2, 0].any()        # lane 0 reads +0.0 from the previous side
    assert not out[:, 1, 63].any() and not out[:, 3, 63].any()      # lane 63 reads +0.0 from the next side


def test_mask_helpers_equal_the_integer_models(hiplib):
    rng = np.random.default_rng(2)
    special = [0, ln.ALL] + [1 << b for b in (15, 16, 20, 21, 31, 32, 41, 42, 47, 48, 62, 63)]
    dense = [int(x) for x in rng.integers(0, 1 << 64, 300, dtype=U64)]
    sparse = [ln.mask_of(rng.choice(64, int(rng.integers(1, 4)), replace=False)) for _ in range(300)]
    pairs = [(m, need) for m in special for need in special] + [(m, need) for m in special for need in sparse[:20] + dense[:5]]
    pairs += [(m, need) for need in special for m in sparse[:20] + dense[:5]]
    pairs += list(zip(dense, sparse)) + list(zip(sparse, dense)) + list(zip(sparse, sparse[::-1])) + list(zip(dense, dense[::-1]))
    pairs += [(m, m) for m in sparse[:50]] + [(m, ln.ALL & ~m) for m in sparse[:50]] + [(m & need, need) for m, need in zip(dense[:100], sparse[:100])]
    rows = np.zeros((len(pairs), 2, 64), U64)
    rows[:, :, 1:] = 0x5555555555555555      # (only lane 0's word is read)
    rows[:, 0, 0] = np.array([m for m, _ in pairs], U64)
    rows[:, 1, 0] = np.array([need for _, need in pairs], U64)
    out = probe(hiplib, "MASK", rows)
    verdicts = set()
    for j, (m, need) in enumerate(pairs):
        d0, d1 = ln.seg_dead32(need)
        want = [ln.seg_uniform(m & ln.seg_desig(21), 21), ln.seg_covered(m, need, 16), ln.seg_covered(m, need, 32), ln.seg_covered(m, need, 64),
                d0, d1, ln.seg_covered32(m, d0, d1)]
        for k, wk in enumerate(want):
            assert np.all(out[j, k] == U64(int(wk))), (hex(m), hex(need), k)
        assert np.array_equal(out[j, 7], ln.lanes(m).astype(U64)) and np.all(out[j, 8] == U64(m)), hex(m)      # mask -> predicate -> ballot
        assert want[2] == want[6]
        verdicts.add(tuple(want[1:4]))
    assert len(verdicts) == 4, verdicts      # (covered at 16 implies at 32 implies at 64: TTT, FTT, FFT, FFF -- all of them occur)


def test_screen_theta_has_the_models_bits(hiplib):
    """on the thresholds of test_lane_screen_cpu.py: zero, subnormal and infinite ones among them"""
    rng = np.random.default_rng(20)
    n = 200000
    p, scale = _partials(rng, n)
    tol2, floor2 = _thresholds(rng, p, scale)
    assert (tol2 == 0).any() and (floor2 == 0).any() and np.isinf(floor2).any() and ((tol2 > 0) & (tol2 < 2.0 ** -1022)).any()
    # ... and one wave more in which BOTH are below the screen's lower limit 2^-1000 (zero, subnormal, the smallest normals)
    low = np.concatenate([[0.0, 5e-324, 2.0 ** -1023, 2.0 ** -1022, 2.0 ** -1001], 2.0 ** -rng.uniform(1001, 1074, 59)])
    tol2, floor2 = np.concatenate([tol2, low]), np.concatenate([floor2, low[::-1]])
    pad = -len(tol2) % 64
    t, f = np.concatenate([tol2, np.zeros(pad)]).reshape(-1, 64), np.concatenate([floor2, np.zeros(pad)]).reshape(-1, 64)
    out = f64(probe(hiplib, "THETA", np.stack([w64(t), w64(f)], axis=1)))[:, 0]
    want = ln.theta(t, f)
    assert same_bits(out, want).all()
    assert (want == 2.0 ** -1000).any() and np.isinf(want).any()


def arith(hiplib, a, b, c, m=None, ok=None, fa=None, fb=None, fc=None):
    """one launch of the ARITH group on [n][64] inputs -> [n][17][64] words"""
    n = a.shape[0]
    m = np.full((n, 64), -1) if m is None else m
    ok = np.ones((n, 64), bool) if ok is None else ok
    flags = (np.asarray(m).astype(np.int64) & 0xffffffff).astype(U64) | (np.asarray(ok).astype(U64) << U64(32))
    fa, fb, fc = (np.zeros((n, 64), np.float32) if x is None else x for x in (fa, fb, fc))
    return probe(hiplib, "ARITH", np.stack([w64(a), w64(b), w64(c), flags, w32(fa), w32(fb), w32(fc)], axis=1))


def odd_values(rng, n, dtype):
    """[n][64]: NaNs with payloads (quiet), infinities, signed zeros, ordinary numbers (fp64: beyond both ends of fp32's range too)"""
    decades = 60 if dtype is np.float64 else 30
    v = (rng.standard_normal((n, 64)) * 10.0 ** rng.uniform(-decades, decades, (n, 64))).astype(dtype)
    kind = rng.integers(0, 8, (n, 64))
    v[kind == 0] = np.nan
    v[kind == 1] = np.inf
    v[kind == 2] = -np.inf
    v[kind == 3] = -0.0
    v[kind == 4] = 0.0
    ut, quiet = (U64, 0x7ff8000000000000) if dtype is np.float64 else (U32, 0x7fc00000)
    bits = v.view(ut)
    bits[kind == 0] = (quiet | rng.integers(1, 1 << 20, (n, 64))[kind == 0]).astype(ut)
    return v


def test_keep_if_lds_block_ldz_and_uniform_load(hiplib):
    rng = np.random.default_rng(3)
    n = 64
    a, b, c, fa = odd_values(rng, n, np.float64), odd_values(rng, n, np.float64), odd_values(rng, n, np.float64), odd_values(rng, n, np.float32)
    m = np.where(rng.random((n, 64)) < 0.5, -1, 0)
    ok = rng.random((n, 64)) < 0.5
    out = arith(hiplib, a, b, c, m, ok, fa)
    off = m == 0
    assert off.any() and (~off).any() and (np.isnan(a) & off).any() and (np.isinf(a) & off).any() and (np.isnan(a) & ~ok).any()
    # keep_if: m = 0 gives +0.0 from NaN / inf / anything, m = -1 keeps the bits
    assert np.array_equal(out[:, 0], ln.keep_if(a, m).view(U64)) and not out[:, 0][off].any() and np.array_equal(out[:, 0][~off], w64(a)[~off])
    assert np.array_equal(out[:, 1], ln.keep_if(fa, m).view(U32).astype(U64)) and not out[:, 1][off].any() and np.array_equal(out[:, 1][~off], w32(fa)[~off])
    # lds_block: the record (a, b, c, a, b, c) read back, +0.0 behind ok = false whatever was read
    for l, src in enumerate((a, b, c, a, b, c)):
        assert np.array_equal(out[:, 6 + l], ln.lds_block(src, ok).view(U64)), l
        assert not out[:, 6 + l][~ok].any()
    # ldz: the fp64 value converted to the kernel's type, +0.0 behind ok = false
    assert np.array_equal(out[:, 12], ln.ldz(a, ok).view(U64)) and not out[:, 12][~ok].any() and not out[:, 13][~ok].any()
    want32 = ln.ldz(a, ok, np.float32)
    nan = np.isnan(want32)
    assert np.array_equal(np.isnan(f32(out[:, 13])), nan) and np.array_equal(out[:, 13][~nan], w32(want32)[~nan])
    assert (np.isinf(want32) & np.isfinite(a)).any() and ((want32 == 0) & (a != 0) & ok).any()      # (overflow and underflow of the conversion are in the set)
    # uniform_load: the table's bits
    assert np.array_equal(out[:, 14], w64(b))


def test_fma3_is_the_correctly_rounded_fma(hiplib):
    rng = np.random.default_rng(4)
    n = 48
    a = rng.standard_normal((n, 64)) * 10.0 ** rng.uniform(-40, 40, (n, 64))
    b = rng.standard_normal((n, 64)) * 10.0 ** rng.uniform(-40, 40, (n, 64))
    c = rng.standard_normal((n, 64)) * 10.0 ** rng.uniform(-80, 80, (n, 64))
    near = rng.random((n, 64)) < 0.6      # c close to -a b: the result is what a product rounded first would lose
    c[near] = -(a * b)[near] * (1.0 + rng.integers(-3, 4, (n, 64))[near] * 2.0 ** -52)
    a[:8] *= 2.0 ** -520
    b[:8] *= 2.0 ** -520                 # products around and inside the subnormal range
    c[:4] = 0.0
    c[4:8] = rng.standard_normal((4, 64)) * 1e-310
    out = f64(arith(hiplib, a, b, c))
    want3 = np.array([[ln.fma(a[w, l], b[w, l], c[w, l]) for l in range(64)] for w in range(n)])
    want3s = np.array([[ln.fma(a[w, 0], b[w, l], c[w, l]) for l in range(64)] for w in range(n)])
    unfused = a * b + c
    print("fma3: %d of %d cases differ from the product rounded first" % (int((~same_bits(want3, unfused)).sum()), want3.size))
    assert (~same_bits(want3, unfused)).sum() > want3.size // 10
    assert same_bits(out[:, 2], want3).all()
    assert same_bits(out[:, 3], want3s).all()


def test_clamp_box_is_fmax_of_fmin(hiplib):
    """as values, NaN-aware (the sign of a zero result is not specified): v NaN, +-inf, +-0, inside, below, above; lo <= hi finite or infinite"""
    boxes = [(-1.0, 1.0), (-np.inf, np.inf), (-np.inf, 2.0), (-3.0, np.inf), (0.0, 0.0), (-0.0, 0.0), (2.5, 2.5), (1e-300, 1e300), (-np.inf, -np.inf),
             (np.inf, np.inf), (-5e-324, 5e-324), (-1e30, -1e-30)]
    vs = [np.nan, np.inf, -np.inf, 0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -7.0, 2.5, 1e-310, -1e-310, 1e301, -1e31, 3e-31, 5e-324]
    rng = np.random.default_rng(6)
    rnd = np.sort(rng.standard_normal((40, 2)) * 10.0 ** rng.uniform(-3, 3, (40, 1)), axis=1)
    cases = [(v, lo, hi) for lo, hi in boxes for v in vs] + [(v, lo, hi) for lo, hi in rnd for v in (np.nan, lo, hi, 0.5 * (lo + hi), lo - 1.0, hi + 1.0)]
    pad = -len(cases) % 64
    arr = np.array(cases + cases[:pad]).reshape(-1, 64, 3)
    v, lo, hi = arr[..., 0].copy(), arr[..., 1].copy(), arr[..., 2].copy()
    assert np.all(lo <= hi)
    with np.errstate(over="ignore", under="ignore"):
        fv, flo, fhi = v.astype(np.float32), lo.astype(np.float32), hi.astype(np.float32)
    assert np.all(flo <= fhi)
    out = arith(hiplib, v, lo, hi, fa=fv, fb=flo, fc=fhi)
    assert np.array_equal(f64(out[:, 4]), ln.clamp_box(v, lo, hi), equal_nan=True)
    assert np.array_equal(f32(out[:, 5]), ln.clamp_box(fv, flo, fhi), equal_nan=True)
    assert not np.isnan(f64(out[:, 4])).any()      # (a NaN v leaves the box's upper bound: minnum drops it)


def ulp_of(q):
    """of a positive rational in fp64's normal range: 2^(floor(log2 q) - 52)"""
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if q < Fraction(2) ** e:
        e -= 1
    return Fraction(2) ** (e - 52)


def test_fast_div_is_within_one_ulp_of_the_quotient(hiplib):
    """biconvex_lanes.h: "a / b to ~1 ulp".  Normal operands, b > 0, normal results; quotients near 1 and near powers of two among them.
    The bound asserted is the header's claim, one ulp of the exact quotient; the fp32 overload is the correctly rounded division."""
    rng = np.random.default_rng(8)
    n = 96
    b = np.abs(rng.standard_normal((n, 64))) * 10.0 ** rng.uniform(-100, 100, (n, 64)) + 1e-200
    a = rng.standard_normal((n, 64)) * 10.0 ** rng.uniform(-100, 100, (n, 64))
    k = rng.integers(-4, 5, (n, 64))
    a[:24] = b[:24] * (1.0 + k[:24] * 2.0 ** -52)                                          # quotients within a few ulp of 1
    a[24:48] = b[24:48] * 2.0 ** rng.integers(-60, 60, (24, 64)) * (1.0 + k[24:48] * 2.0 ** -52) * rng.choice([1.0, -1.0], (24, 64))      # ... of a power of two
    b[48:56] = rng.integers(1, 1 << 20, (8, 64)).astype(np.float64)
    a[48:56] = b[48:56] * rng.integers(-1000, 1000, (8, 64))                               # exact quotients
    a[56:64] = np.nextafter(1.0, 2.0) * rng.choice([1.0, 2.0 ** 40, 2.0 ** -40], (8, 64))
    b[56:64] = 1.0 + rng.integers(1, 1 << 30, (8, 64)) * 2.0 ** -52                        # just above 1: quotients just below a power of two
    fa = (rng.standard_normal((n, 64)) * 10.0 ** rng.uniform(-10, 10, (n, 64))).astype(np.float32)
    fb = (rng.standard_normal((n, 64)) * 10.0 ** rng.uniform(-10, 10, (n, 64))).astype(np.float32)
    fa[:24] = fb[:24] * (np.float32(1.0) + k[:24].astype(np.float32) * np.float32(2.0 ** -23))
    out = arith(hiplib, a, b, a, fa=fa, fb=fb)
    got, got32 = f64(out[:, 15]), f32(out[:, 16])
    worst, inexact, total = Fraction(0), 0, 0
    for w in range(n):
        for l in range(64):
            q = Fraction(a[w, l]) / Fraction(b[w, l])
            if q == 0:
                assert got[w, l] == 0.0
                continue
            assert 2.0 ** -1000 < abs(q) < 2.0 ** 1000
            err = abs(Fraction(float(got[w, l])) - q) / ulp_of(abs(q))
            worst = max(worst, err)
            inexact += got[w, l] != ln.round_fraction(q)
            total += 1
            fq = Fraction(float(fa[w, l])) / Fraction(float(fb[w, l]))
            if 2.0 ** -120 < abs(fq) < 2.0 ** 120:
                assert got32[w, l].view(U32) == ln.round_fraction(fq, np.float32).view(U32), (w, l)
    print("fast_div: largest error %.4f ulp of the exact quotient over %d cases; %d not correctly rounded" % (float(worst), total, inexact))
    assert worst <= 1


def test_banded_decisions_equal_the_model(hiplib):
    """the one-problem-per-wave kernel's fp32 shortcut: wave sums of g2 and cv in float32, the 16-lane swap that pairs g2's rows with cv's"""
    rng = np.random.default_rng(10)
    n = 1500
    tol2 = 1e-10
    g2 = np.stack([wide(rng, 64) for _ in range(n)]) * 10.0 ** rng.uniform(-30, -8, (n, 1))
    Lh = 10.0 ** rng.uniform(-1, 7, n)
    third = np.arange(n) % 3 == 0
    s = g2.sum(axis=1)
    g2[third] *= (tol2 / np.maximum(s[third], 1e-300) * (1.0 + rng.normal(0, 3e-5, third.sum())))[:, None]      # g2 within a few 1e-5 of tol^2
    cv = g2 * np.abs(rng.normal(1.0, 0.3, (n, 64)))
    scale = np.where(np.arange(n) % 3 == 1, 1.0 + rng.normal(0, 3e-5, n), 1.0 + rng.normal(0, 0.5, n))
    cv *= (Lh * g2.sum(axis=1) / np.maximum(cv.sum(axis=1), 1e-300) * scale)[:, None]                             # cv near the retry threshold
    g2[-1, 5], cv[-2, 40], g2[-3, 63], g2[-4], cv[-5], g2[-6] = np.nan, np.nan, np.inf, 1e-40, 1e35, 0.0         # NaN, inf, out of range: not clear
    tol = np.full(n, tol2)
    rows = np.stack([w64(g2), w64(cv), w64(np.repeat(Lh[:, None], 64, 1)), w64(np.repeat(tol[:, None], 64, 1))], axis=1)
    rows[:, 2:, 1:] = w64(np.array([np.nan]))[0]      # (only lane 0's Lh and tol2 are read)
    out = probe(hiplib, "BANDED", rows)
    want = np.array([ln.banded_decisions(g2[w], cv[w], Lh[w], tol2) for w in range(n)])
    for k in range(3):
        assert np.array_equal(out[:, k], np.repeat(want[:, k:k + 1], 64, 1).astype(U64)), k
    print("banded_decisions: clear in %d of %d waves, retry in %d, finished in %d" % (want[:, 0].sum(), n, want[:, 1].sum(), want[:, 2].sum()))
    assert n // 4 < want[:, 0].sum() < n and not want[-6:, 0].any() and 0 < want[:, 1].sum() < n and 0 < want[:, 2].sum() < n
