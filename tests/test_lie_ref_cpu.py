"""oracle/rbd_np.py held to tests/golden/lie_ref.npz: the rows and caps of tests/test_lie_ref_gpu.py, so that the oracle the device is
compared with elsewhere (tests/test_rbd_gpu.py, the IK parity tests) is itself held to 60-digit evaluations of the definitions and not
only to the device.  The three elementary ops have no restatement in the oracle: it calls numpy's, which are what is run here.
With mpmath at hand every 16th row of the fixture is derived again (a stale file).  No GPU."""
import numpy as np
import pytest

from oracle import rbd_np as rb
from tests import lie_ref

ROWS = lie_ref.load()


def _unit_q(q):
    return q / np.linalg.norm(q)


class _Free:      # the free-flyer alone
    nq, nv = 7, 6


def _diff(x):
    """the oracle's own entry points, as the IK twins call them: the base block of difference and of state_jdiff_second"""
    x0, x1 = np.concatenate([x[0:7], np.zeros(6)]), np.concatenate([x[7:14], np.zeros(6)])
    return np.concatenate([rb.difference(_Free, x0[:7], x1[:7]), rb.state_jdiff_second(_Free, x0, x1)[:6, :6].ravel()])


def _integrate(x, ref):
    out = rb.integrate(_Free, x[:7], x[7:13])
    # R_to_quat returns one of the two quaternions of the rotation, not necessarily the product's: the one on the reference's side
    return np.concatenate([out[:3], out[3:] if out[3:] @ ref[3:] >= 0 else -out[3:]])


def _sincos(x):
    return np.array([np.sin(x[0]), np.cos(x[0])])


ORACLE = {
    "sincos": _sincos,
    "rcp_rsqrt": lambda x: np.array([1.0 / x[0], 1.0 / np.sqrt(x[0])]),
    "atan2_pos": lambda x: np.array([np.arctan2(x[0], x[1])]),
    "exp6": lambda x: np.concatenate([rb.exp6(x)[0].ravel(), rb.exp6(x)[1]]),
    "jexp3": lambda x: rb.jexp3(x).ravel(),
    "jlog3": lambda x: rb.jlog3(x).ravel(),
    "q_left": lambda x: rb._q_left(x[:3], x[3:]).ravel(),
    "jexp6": lambda x: rb.jexp6(x).ravel(),
    "log3_q": lambda x: rb.log3(rb.quat_to_R(_unit_q(x))),
    "diff": _diff,
}


def test_fixture_has_every_op_whole():
    for op, (_, nin, _, nref, _) in lie_ref.OPS.items():
        r = ROWS[op]
        n = len(r["in"])
        assert 0 < n <= 512 and r["in"].shape == (n, nin) and r["ref"].shape == (n, nref) == r["alt"].shape, op
        assert r["unit"].shape in ((n, 1), (n, nref)) and np.all(r["unit"] > 0) and np.isfinite(r["unit"]).all(), op
        assert all(np.isfinite(r[k]).all() for k in ("in", "ref", "alt")), op
        if op not in ("sincos", "rcp_rsqrt", "atan2_pos"):
            # no vacuous unit: a unit is roundings and last bits of inputs, 1e-16 of the row's scale times its condition -- never a branch jump
            scale = np.maximum(np.abs(r["ref"]).max(axis=1), np.abs(r["in"]).max(axis=1))
            assert np.all(r["unit"][:, 0] <= 1e-12 * scale), (op, np.nonzero(r["unit"][:, 0] > 1e-12 * scale)[0])


@pytest.mark.parametrize("op", list(lie_ref.OPS))
def test_oracle_within_the_caps(op):
    rows = ROWS[op]
    with np.errstate(all="ignore"):
        if op == "integrate":
            got = np.array([_integrate(x, ref) for x, ref in zip(rows["in"], rows["ref"])])
        else:
            got = np.array([ORACLE[op](x) for x in rows["in"]])
    if op == "diff":      # the Jacobian against the one of the axis sign that the difference took
        assert np.isfinite(got).all()
        lie_ref.report(op, lie_ref.units_diff(got[:, :6], got[:, 6:], rows), rows, "oracle/rbd_np.py")
    else:
        lie_ref.check(op, got, rows, "oracle/rbd_np.py")


def test_plan_builder_log3_within_the_cap():
    """the private log3 of bunmpc_amd/problems.py (the numpy plan builder's amom), a batch at a time"""
    from bunmpc_amd import problems
    rows = ROWS["log3_q"]
    R = np.array([rb.quat_to_R(_unit_q(q)) for q in rows["in"]])
    lie_ref.check("log3_q", problems._log3_batch(R), rows, "problems._log3_batch")


@pytest.mark.parametrize("op", list(lie_ref.OPS))
def test_fixture_is_what_the_generator_writes(op):
    pytest.importorskip("mpmath")
    from tests.golden import make_golden_lie as gen
    rows = ROWS[op]
    # the rows: to the last bits of this machine's sin, cos and pow, which place them; what is derived from the file's rows: exactly
    mine = gen.inputs()[op]
    assert mine.shape == rows["in"].shape and np.allclose(mine, rows["in"], rtol=1e-14, atol=1e-15)
    for i in range(0, len(rows["in"]), 16):
        ref, alt, unit = gen.reference(op, rows["in"][i])
        assert np.array_equal(ref, rows["ref"][i]) and np.array_equal(alt, rows["alt"][i]) and np.array_equal(unit, rows["unit"][i]), (op, i)
