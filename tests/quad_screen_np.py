"""Numpy model of the quad stage of the certified loops' screen (biconvex_lanes.h: quad_theta_f32, quad_sum_f32, quad_screen): the
lane's partial of the squared step converted to fp32 and summed over its DPP quad, against theta enlarged by a margin.  A restatement
for tests/test_quad_screen_cpu.py; every operation in the kernel's order on np.float32 / np.float64, round to nearest."""
import numpy as np

MARGIN = 1.0 + 2.0 ** -20
FLOOR = np.float32(2.0 ** -100)


def quad_theta(theta):
    """quad_theta_f32: theta (1 + 2^-20) rounded to fp32, at least 2^-100; +inf stays +inf"""
    with np.errstate(over="ignore"):
        return np.fmax(np.float32(np.float64(theta) * MARGIN), FLOOR)      # (fmaxf: a NaN operand is dropped)


def quad_sum(g2):
    """quad_sum_f32 on [..., lanes] partials (lanes a multiple of 4): q = float(g2); q += q[lane ^ 1]; q += q[lane ^ 2]"""
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.asarray(g2, np.float64).astype(np.float32)
        lane = np.arange(q.shape[-1])
        q = q + q[..., lane ^ 1]
        q = q + q[..., lane ^ 2]
    return q


def quad_screen(g2, theta):
    """the lanes whose quad settles their segment's iteration"""
    with np.errstate(invalid="ignore"):
        return quad_sum(g2) > quad_theta(theta)
