"""The lane helpers of the centroidal kernels (bunmpc_amd/csrc/biconvex_lanes.h) restated in numpy and Python integers: one array per
wave of 64 lanes, additions in the order of the DPP / permlane butterflies and in the kernel's number type, masks as Python ints.  The
CPU proofs (test_step_decisions_cpu.py, test_lane_screen_cpu.py, test_term_screen_cpu.py) argue about these functions, and
test_lane_probe_gpu.py holds the device to them bit for bit (bmpc_probe_lanes), so what is proved is what the hardware does."""
import os
import sys
from fractions import Fraction

import numpy as np

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)
from screen_rate import butterfly_sum32, theta  # noqa: E402,F401  (seg_sum<32> on [..., 32] partials; screen_theta)

LANES = np.arange(64)
ALL = (1 << 64) - 1


def _partner(kind):
    if kind == "xor1":
        return LANES ^ 1
    if kind == "xor2":
        return LANES ^ 2
    if kind == "half_mirror":
        return (LANES & ~7) | (7 - (LANES & 7))
    return (LANES & ~15) | (15 - (LANES & 15))      # row_mirror


def _rows(v):
    with np.errstate(invalid="ignore", over="ignore"):
        for kind in ("xor1", "xor2", "half_mirror", "mirror"):
            v = v[..., _partner(kind)] + v     # v_add_f32_dpp v, v(dpp), v
    return v


def _swap2(a, b, width):
    """x = permlane{16,32}_swap(a, b); x[0] + x[1]: the odd blocks of `width` lanes of a change places with the even blocks of b"""
    lo = (LANES // width) % 2 == 0
    even = np.where(lo, a, b[..., (LANES - width) % 64])
    odd = np.where(lo, a[..., (LANES + width) % 64], b)
    with np.errstate(invalid="ignore", over="ignore"):
        return even + odd


def _swap(v, width):
    """x = permlane{16,32}_swap(v, v); x[0] + x[1]: the two blocks of `width` lanes of each pair add"""
    return _swap2(v, v, width)


def _is_p(lane):
    row = lane >> 4
    return row == 0 or lane // 21 == (16 * row) // 21 + 1


IS_P = np.array([_is_p(int(l)) for l in LANES])


def seg_sum(v, lpp):
    """the kernels' segment sum of v ([..., 64] lanes, float32 or float64) in their order of additions; valid at desig(lpp)"""
    zero = v.dtype.type(0)
    if lpp == 21:
        p = _rows(np.where(IS_P, v, zero))
        q = _rows(np.where(IS_P, zero, v))
        bc = np.where(LANES >= 16, p[..., np.maximum((LANES & ~15) - 1, 0)], zero)      # row_bcast:15; row 0 keeps the old value 0
        with np.errstate(invalid="ignore", over="ignore"):
            return bc + q
    v = _rows(v)
    if lpp >= 32:
        v = _swap(v, 16)
    if lpp >= 64:
        v = _swap(v, 32)
    return v


def seg_sum2(a, b, lpp):
    """seg_sum2<LPP> / seg_sum2_f32<LPP> (by the dtype): each sum has seg_sum's order of additions"""
    return seg_sum(a, lpp), seg_sum(b, lpp)


def seg_sum1(a, lpp):
    """seg_sum1<LPP> / seg_sum1_f32<LPP>"""
    return seg_sum(a, lpp)


def seg_sum_all(v, lpp):
    """seg_sum<LPP>: the sum in EVERY lane (LPP = 21: the designated lanes' values read back by their segments; lane 63 reads segment 2's)"""
    s = seg_sum(v, lpp)
    return s[..., np.array([16, 32, 48])[np.minimum(LANES // 21, 2)]] if lpp == 21 else s


def desig(lpp):
    return np.array([16, 32, 48]) if lpp == 21 else np.arange(0, 64, lpp)


def segments(lpp):
    return [np.arange(21 * k, 21 * k + 21) for k in range(3)] if lpp == 21 else [np.arange(s, s + lpp) for s in range(0, 64, lpp)]


# ---- one-lane shifts (wave_shr:1 / wave_shl:1 with bound_ctrl: the wave's ends read +0.0); bits are moved, not values

def from_prev(v):
    out = np.zeros_like(v)
    out[..., 1:] = v[..., :-1]
    return out


def from_next(v):
    out = np.zeros_like(v)
    out[..., :-1] = v[..., 1:]
    return out


# ---- lane masks: Python ints of 64 bits

def mask_of(lanes):
    m = 0
    for l in lanes:
        m |= 1 << int(l)
    return m


def seg_desig(lpp):
    return mask_of([16, 32, 48]) if lpp == 21 else ALL


def seg21_spread(m):
    seg = (1 << 21) - 1
    return (seg if (m >> 16) & 1 else 0) | (seg << 21 if (m >> 32) & 1 else 0) | (seg << 42 if (m >> 48) & 1 else 0)


def seg_uniform(m, lpp):
    return seg21_spread(m) if lpp == 21 else m


def seg_covered(have, need, lpp):
    """does every lpp-lane segment (16, 32, 64) with a bit in need have a bit in have?"""
    seg = (1 << lpp) - 1
    return all((need >> s) & seg == 0 or (have >> s) & seg != 0 for s in range(0, 64, lpp))


def seg_dead32(need):
    return (0xffffffff if need & 0xffffffff == 0 else 0), (0xffffffff if need >> 32 == 0 else 0)


def seg_covered32(have, d0, d1):
    return min((have & 0xffffffff) | d0, (have >> 32) | d1) != 0


def lanes(m):
    """the per-lane predicate of a mask"""
    return np.array([(m >> int(l)) & 1 == 1 for l in LANES])


# ---- small arithmetic helpers

def keep_if(v, m):
    """v where the 32-bit word m is all ones, +0.0 where it is 0: an and of the bits with m (both halves of a double)"""
    v = np.asarray(v)
    m = np.asarray(m).astype(np.int64) & 0xffffffff
    if v.dtype == np.float64:
        return (v.view(np.uint64) & (m | (m << 32)).astype(np.uint64)).view(np.float64)
    return (v.view(np.uint32) & m.astype(np.uint32)).view(np.float32)


def clamp_box(v, lo, hi):
    """max(min(v, hi), lo) with minnum / maxnum: a NaN operand is dropped (the sign of a zero result is not specified)"""
    return np.fmax(np.fmin(v, hi), lo)


def round_fraction(x, dtype=np.float64):
    """the rational x rounded to the nearest number of dtype, ties to even: the correctly rounded result of an exact operation.
    (A zero comes back as +0.0; overflow is not handled: the callers stay inside the normal range.)"""
    dtype = np.dtype(dtype).type
    p, emin = (53, -1022) if dtype is np.float64 else (24, -126)
    x = Fraction(x)
    if x == 0:
        return dtype(0.0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()      # 2^(e-1) < a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1                                                      # now 2^e <= a < 2^(e+1)
    q = max(e, emin) - (p - 1)                                      # the weight of the last place (subnormals: fixed)
    scaled = a / Fraction(2) ** q
    n = scaled.numerator // scaled.denominator
    rest = scaled - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n & 1):
        n += 1
    r = np.ldexp(np.float64(n), q)                                  # n < 2^53 and the result is representable: exact
    assert Fraction(float(r)) == n * Fraction(2) ** q
    out = dtype(r)
    assert Fraction(float(out)) == Fraction(float(r))
    return -out if x < 0 else out


def fma(a, b, c):
    """fl(a b + c) of finite numbers, one rounding: the exact rational value rounded once"""
    dtype = np.asarray(a).dtype.type
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x != 0:
        return round_fraction(x, dtype)
    # an exact zero: -0 only if both addends are negative zeros (round to nearest), a sum of opposite non-zeros is +0
    prod_zero = float(a) == 0.0 or float(b) == 0.0
    prod_neg = bool(np.signbit(a)) != bool(np.signbit(b))
    return dtype(-0.0) if prod_zero and prod_neg and float(c) == 0.0 and np.signbit(c) else dtype(0.0)


def fast_div(a, b):
    """the correctly rounded quotient of finite numbers, b != 0: what fast_div approximates in fp64 and is in fp32"""
    return round_fraction(Fraction(float(a)) / Fraction(float(b)), np.asarray(a).dtype.type)


def ulp(x):
    """the distance between |x| and the next larger fp64 number"""
    x = np.abs(np.asarray(x, np.float64))
    return np.nextafter(x, np.inf) - x


def lds_block(v, ok):
    """the values read, +0.0 where the lane has no business with them (a select: NaN does not pass)"""
    return np.where(ok, v, np.zeros_like(v))


def ldz(v, ok, dtype=np.float64):
    """the fp64 value in memory converted to the kernel's type, +0.0 behind ok = false"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(ok, np.asarray(v, np.float64).astype(dtype), dtype(0))


def banded_decisions(g2, cv, Lh, tol2):
    """banded_decisions (the one-problem-per-wave kernel): WAVE sums of g2 and cv in float32 -- the row butterflies, one 16-lane swap of
    g2's rows against cv's (rows 0 / 2 then hold g2 over a row pair, rows 1 / 3 cv), one 32-lane swap, lane 0 = sum of g2, lane 16 = sum
    of cv -- and the two decisions with their bands.  g2, cv: float64 [64]; returns (clear, retry, finished) as Python bools."""
    with np.errstate(over="ignore", invalid="ignore"):
        a, b = _rows(np.asarray(g2, np.float64).astype(np.float32)), _rows(np.asarray(cv, np.float64).astype(np.float32))
        w = _swap(_swap2(a, b, 16), 32)
        g2w, cvw = w[0], w[16]
        g2s, cvs = np.float64(g2w), np.float64(cvw)
        rhs = np.float64(Lh) * g2s
        retry, finished = bool(cvs > rhs), bool(g2s < np.float64(tol2))
        ordinary = bool(g2w > np.float32(1e-30)) and bool(g2w < np.float32(1e30)) and bool(cvw < np.float32(1e30))
        clear = ordinary and bool(np.abs(cvs - rhs) > 1e-5 * rhs) and bool(np.abs(g2s - np.float64(tol2)) > 1e-5 * np.float64(tol2))
    return clear, retry, finished
