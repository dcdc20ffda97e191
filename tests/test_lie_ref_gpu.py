"""The SE(3) primitives of csrc/rbd_device.h on the device against tests/golden/lie_ref.npz: 60-digit evaluations of the definitions at the
edges -- either side of every series cut, the decade above each, rotations up to and at pi, unnormalised and opposite quaternions, the
multiples of pi/2, powers of two -- each row with the unit any float64 routine is allowed there (tests/golden/make_golden_lie.py).
tests/test_rbd_gpu.py compares the same routines with oracle/rbd_np.py, which evaluates the same expressions with the same cut-overs:
that pins the transcription, this pins the arithmetic.  The probe is a kernel of its own in csrc/lie_probe.hip behind a test-only entry
point that no header declares, bound here by name; one launch per op, every row of the fixture.

Measured on an MI355X, worst row in units (cap), the routines as they were before this reference existed -> as they are:
exp6 63 -> 0.99 (8), jexp3 124 -> 0.79 (8), jlog3 1.7e5 -> 0.66 (8), q_left 5.3e3 -> 1.3 (32), jexp6 4.8e3 -> 0.84 (32),
log3_q 5.7e4 -> 1.3 (8), state_diff<false> 2.6e5 -> 1.8 (32), the Jl of state_diff<true> 5.5e4 -> 0.71 (32), state_integrate 26 -> 0.91
(32); state_diff_q 0.96, state_integrate_q 0.58, sincos_fast, rcp_fast, rsqrt_fast and atan2_pos 1.0 were within their caps and are
unchanged.  EXPERIMENTS.md has the rows."""
import ctypes as C

import numpy as np
import pytest

from bunmpc_amd import _lib
from tests import lie_ref

pytestmark = pytest.mark.gpu

ROWS = lie_ref.load()


def bind(hiplib):
    fn = hiplib.bmpc_probe_lie
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int]
    return fn


def probe(hiplib, op, rows):
    number, nin, nout, _, _ = lie_ref.OPS[op]
    x = np.ascontiguousarray(rows, np.float64)
    assert x.shape[1] == nin
    out = np.full((len(x), nout), np.nan)
    assert bind(hiplib)(number, x.ctypes.data, x.size, out.ctypes.data, out.size, len(x)) == _lib.OK
    return out


@pytest.mark.parametrize("op", list(lie_ref.OPS))
def test_device_within_the_caps(hiplib, op):
    rows = ROWS[op]
    got = probe(hiplib, op, rows["in"])
    assert np.isfinite(got).all(), "%s: a value that is not finite" % op
    if op == "diff":      # each difference on its own (at pi the two may choose opposite axes); Jl is built from state_diff_q's
        lie_ref.report(op, lie_ref.units_diff(got[:, :6], got[:, 12:], rows), rows, "state_diff_q, its Jl")
        lie_ref.check(op, got[:, 6:12], rows, "state_diff<false>", slice(0, 6))
    elif op == "integrate":
        lie_ref.check(op, got[:, :7], rows, "state_integrate_q")
        lie_ref.check(op, got[:, 7:], rows, "state_integrate")
    else:
        lie_ref.check(op, got, rows, "rbd_device.h")


def test_bad_arguments_are_refused(hiplib):
    fn = bind(hiplib)
    buf = (C.c_double * 64)()
    for args in ((-1, buf, 6, buf, 12, 1), (11, buf, 6, buf, 12, 1), (3, None, 6, buf, 12, 1), (3, buf, 6, None, 12, 1), (3, buf, 0, buf, 0, 0),
                 (3, buf, -6, buf, -12, -1), (3, buf, 5, buf, 12, 1), (3, buf, 6, buf, 11, 1), (3, buf, 12, buf, 12, 1), (3, buf, 6, buf, 12, 2),
                 (9, buf, 14, buf, 42, 1)):
        assert fn(*args) == _lib.BAD_ARG, (args[0],) + args[2::2]
    assert fn(3, buf, 6, buf, 12, 1) == _lib.OK
