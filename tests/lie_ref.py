"""What tests/test_lie_ref_cpu.py and tests/test_lie_ref_gpu.py share: the ops of the SE(3) probe (bmpc_probe_lie, csrc/lie_probe.hip), their
widths, their caps, and the comparison of a routine's rows with tests/golden/lie_ref.npz (written by tests/golden/make_golden_lie.py from
60-digit evaluations of the definitions; the unit of a row is what any float64 routine is allowed there, see that file)."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lie_ref.npz")

# op: (number in the probe, doubles in, doubles the probe writes, doubles of the reference, cap in units)
OPS = {
    "sincos": (0, 1, 2, 2, 2.0),
    "rcp_rsqrt": (1, 1, 2, 2, 2.0),
    "atan2_pos": (2, 2, 1, 1, 4.0),
    "exp6": (3, 6, 12, 12, 8.0),
    "jexp3": (4, 3, 9, 9, 8.0),
    "jlog3": (5, 3, 9, 9, 8.0),
    "q_left": (6, 6, 9, 9, 32.0),
    "jexp6": (7, 6, 36, 36, 32.0),
    "log3_q": (8, 4, 3, 3, 8.0),
    "diff": (9, 14, 48, 42, 32.0),          # the probe: state_diff_q (6), state_diff<false> (6), Jl (36); the reference: the difference once
    "integrate": (10, 13, 14, 7, 32.0),     # the probe: state_integrate_q (7), state_integrate (7); the reference: once
}


def load():
    """{op: {"in": [n][in], "ref": [n][ref], "alt": [n][ref] (the other axis sign where it is free, else a copy of ref), "unit": [n][1 or ref]}}"""
    with np.load(FIXTURE) as z:
        rows = {op: {k: z["%s_%s" % (op, k)] for k in ("in", "ref", "unit")} for op in OPS}
        for op, r in rows.items():
            r["alt"] = r["ref"].copy()
            r["alt"][z[op + "_alt_rows"]] = z[op + "_alt"]
        return rows


def sides(got, rows, cols=slice(None)):
    """per row, the largest error of got [n][columns cols of the reference] in the row's units: (against ref, against alt)"""
    unit = rows["unit"][:, cols] if rows["unit"].shape[1] > 1 else rows["unit"]
    with np.errstate(invalid="ignore"):
        e = np.abs(got - rows["ref"][:, cols]) / unit
        ea = np.abs(got - rows["alt"][:, cols]) / unit
    return np.where(np.isnan(e), np.inf, e).max(axis=1), np.where(np.isnan(ea), np.inf, ea).max(axis=1)


def units(got, rows, cols=slice(None)):
    """... against the nearer of the two references: for ONE quantity that comes from one evaluation of the logarithm"""
    return np.minimum(*sides(got, rows, cols))


def units_diff(d, J, rows):
    """a difference d [n][6] against the nearer reference, and the Jacobian J [n][36] that was built from d against the Jacobian of THAT
    sign (the other one where d is nearer to alt): at a rotation by pi a routine may return either axis, not one axis with the Jacobian
    of the other"""
    e, ea = sides(d, rows, slice(0, 6))
    eJ, eaJ = sides(J, rows, slice(6, 42))
    return np.maximum(np.minimum(e, ea), np.where(ea < e, eaJ, eJ))


def report(op, u, rows, what):
    """every row within the op's cap; prints the worst row"""
    cap = OPS[op][4]
    worst = int(np.argmax(u))
    print("%-10s %-22s worst row %3d of %3d: %8.3f units (cap %g), input %s" % (op, what, worst, len(u), u[worst], cap, np.array2string(rows["in"][worst], precision=17)))
    assert len(u) == len(rows["in"]) and u[worst] <= cap, "%s %s: row %d is off by %.3g units, cap %g" % (what, op, worst, u[worst], cap)
    return u[worst]


def check(op, got, rows, what, cols=slice(None)):
    """every value finite, every row within the op's cap"""
    assert got.shape == rows["ref"][:, cols].shape and np.isfinite(got).all(), "%s %s: a value that is not finite" % (what, op)
    return report(op, units(got, rows, cols), rows, what)
