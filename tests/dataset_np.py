"""A host restatement of the three calls of include/ext/bunmpc_dataset.h, the checker of tests/test_dataset_device_gpu.py (itself held
to bunmpc_amd/dataset.py::Database and to exact arithmetic in tests/test_dataset_device_cpu.py):

  kept_rows   which rows of a (B, R, w) append go in: rows[b] clipped to [0, R], keep[b], and the non-finite rule (a problem whose kept
              rows hold a NaN or an infinity in any given group brings none: simulation.py:513-516, data_collection.py:272-277)
  TwinDatabase.append   the ring, by the reference's row-by-row loop (database.py:121-143)
  moments     mean and population std per column over buffer rows [0, length), as numpy computes them
  batch       [state | goal], action of the rows `index`; (v - mean) / std when normalised; NaN rows outside [0, length)

`fault` (None in the checker) plants one fault for the tests that show the comparisons have teeth."""
import warnings
from fractions import Fraction

import numpy as np

GROUPS = ("states", "vc_goals", "cc_goals", "actions")


def kept_rows(B, R, rows=None, keep=None, drop_nonfinite=False, groups=(), fault=None):
    """(b, r) index arrays of the kept rows, b ascending, r ascending; groups: the given (B, R, w) arrays, scanned by drop_nonfinite"""
    c = np.full(B, R, dtype=np.int64) if rows is None else np.clip(np.asarray(rows, dtype=np.int64), 0, R)
    if keep is not None:
        c = np.where(np.asarray(keep) == 0, 0, c)
    if drop_nonfinite:
        for b in range(B):
            if any(not np.all(np.isfinite(np.asarray(g)[b, :c[b]])) for g in groups):
                c[b] = 0
    if fault == "last_kept_row":
        c = np.maximum(c - 1, 0)
    bs = np.repeat(np.arange(B), c)
    rs = np.concatenate([np.arange(n) for n in c]) if B else np.zeros(0, dtype=np.int64)
    return bs, rs.astype(np.int64)


class TwinDatabase:
    def __init__(self, limit, w_cc=12, fault=None):
        self.limit, self.start, self.length, self.fault = int(limit), 0, 0, fault
        self.buf = dict(states=np.zeros((limit, 43)), vc_goals=np.zeros((limit, 5)), cc_goals=np.zeros((limit, w_cc)), actions=np.zeros((limit, 12)))

    def append(self, states, actions, vc_goals=None, cc_goals=None, rows=None, keep=None, drop_nonfinite=False):
        """arrays (n, w) or (B, R, w); returns the number of kept rows"""
        if vc_goals is None and cc_goals is None:
            raise ValueError("both vc_goals and cc_goals cant be empty!")
        given = {k: np.asarray(v, dtype=np.float64) for k, v in (("states", states), ("actions", actions), ("vc_goals", vc_goals), ("cc_goals", cc_goals))
                 if v is not None}
        given = {k: (v[:, None, :] if v.ndim == 2 else v) for k, v in given.items()}
        B, R = given["states"].shape[:2]
        bs, rs = kept_rows(B, R, rows, keep, drop_nonfinite, list(given.values()), self.fault)
        limit = self.limit
        for b, r in zip(bs, rs):                      # database.py:121-143, row by row
            if self.length < limit:
                self.length += 1
            else:
                self.start = (self.start + 1) % limit
            slot = (self.start + self.length - 1) % limit
            if self.fault == "late_wrap":
                slot = (self.start + self.length - 1) % (limit + 1) % limit
            for k, v in given.items():
                self.buf[k][slot] = v[b, r]
        return len(bs)

    def moments(self):
        """{group: (mean, std)} of states and cc_goals over rows [0, length) (database.py:187-213)"""
        n = self.limit if self.fault == "mean_over_limit" else self.length
        out = {}
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # an empty data set: NaN, as the reference gets
            for k in ("states", "cc_goals"):
                a = self.buf[k][:self.length]
                if n != self.length:
                    out[k] = (a.sum(axis=0) / n, np.sqrt(((a - a.sum(axis=0) / n) ** 2).sum(axis=0) / n))
                else:
                    out[k] = (np.mean(a, axis=0), np.std(a, axis=0)) if a.shape[1] else (np.zeros(0), np.zeros(0))
        return out

    def batch(self, index, goal_type="cc", normalise=True, stats=None):
        """stats: {group: (mean, std)} as moments() returns (default: its own)"""
        index = np.asarray(index, dtype=np.int64)
        stats = self.moments() if stats is None and normalise else stats
        goal = "cc_goals" if goal_type == "cc" else "vc_goals"
        wx = 43 + self.buf[goal].shape[1]
        x, y = np.full((len(index), wx), np.nan), np.full((len(index), 12), np.nan)
        ok = (index >= 0) & (index < self.length)
        s, g = self.buf["states"][index[ok]], self.buf[goal][index[ok]]
        if normalise:
            with np.errstate(all="ignore"):
                s = (s - stats["states"][0]) / stats["states"][1]
                g = (g - stats["cc_goals"][0]) / stats["cc_goals"][1] if goal_type == "cc" else (g - 0.0) / 1.0
        x[ok], y[ok] = np.hstack([s, g]), self.buf["actions"][index[ok]]
        return x, y


# ---- exact arithmetic: what the moments are held to -----------------------------------------------------------------------------------

U = Fraction(1, 2 ** 53)


def exact_moments(a):
    """per column of a (n, w): (mean, variance, mean |x|) as Fractions"""
    a = np.asarray(a, dtype=np.float64)
    n, out = a.shape[0], []
    for col in a.T:
        xs = [Fraction(float(v)) for v in col]
        m = sum(xs) / n
        out.append((m, sum((x - m) ** 2 for x in xs) / n, sum(abs(x) for x in xs) / n))
    return out


def moment_violations(mean, std, exact, n, factor=1):
    """Columns whose mean or std misses `factor` times the bounds, with u = 2^-53, a = mean |x|, s2 the exact variance, any summation order:
        |mean - exact| <= n u a                          (a sum of n terms, then one division)
        |std^2 - s2|   <= (n + 4) u s2 + (n u a)^2       (sum (x - m')^2 = sum (x - m)^2 + n (m - m')^2 exactly, plus the relative
                                                          error of a sum of n non-negative terms, the subtraction, the square, the
                                                          division and the square root)
    which for a constant column c is std <= n u |c|.  Compared as Fractions: nothing here rounds."""
    bad = []
    for j, (m, s2, a) in enumerate(exact):
        em = abs(Fraction(float(mean[j])) - m)
        ev = abs(Fraction(float(std[j])) ** 2 - s2)
        bm, bv = factor * n * U * a, factor * ((n + 4) * U * s2 + (n * U * a) ** 2)
        print("column %d: mean error %.3e of bound %.3e, variance error %.3e of bound %.3e" % (j, em, bm, ev, bv))
        if not (em <= bm and ev <= bv):
            bad.append(j)
    return bad
