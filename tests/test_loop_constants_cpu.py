"""Where the dispatch takes the loop-constants build of the benchmark's kernel (bmpc_set_loop_constants_in_lds): the
two-waves-per-SIMD build of the 32-lane, four-feet, harness-form fp64 kernel whose certified FISTA loops keep x_k in registers and read
18 constants of the phase from LDS.  Asked of bmpc_biconvex_plan_launch and of the fit function; no GPU."""
import ctypes as C

import pytest

from bunmpc_amd import _lib
from tests import dispatch_rows as dr

SIMDS = 1024


def _row(**kw):
    row = dict(E=4, k=21, B=4096, form="harness", precision=0, num_iters=10, shape="diag", knob=None, value=0)
    row.update(kw)
    return row


def _plan(hiplib, row, mode, shape=None):
    d, out = dr.descriptor(row), _lib.LaunchPlan()
    with dr.knob(hiplib, "loop_constants_in_lds", mode), dr.knob(hiplib, row["knob"], row["value"]):
        rc = hiplib.bmpc_biconvex_plan_launch(C.byref(d), dr.SHAPES[row["shape"]] if shape is None else shape, SIMDS, C.byref(out))
    return rc, out


def _record(out):
    return out.status, out.kernel, out.lanes_per_problem, out.waves_per_simd, out.steal, out.steal_waves


@pytest.mark.parametrize("k", [17, 18, 19, 20, 21])
def test_planned_where_the_two_waves_build_is_and_it_fits(hiplib, k):
    """B = 4096 on 1024 SIMDs: 2048 waves of two problems, more than the chip has SIMDs"""
    rc, on = _plan(hiplib, _row(k=k), 1)
    rc0, off = _plan(hiplib, _row(k=k), 0)
    assert rc == 0 and rc0 == 0
    assert _record(off) == (0, b"biconvex_admm_kernel", 32, 2, 0, 0) and off.loop_constants_in_lds == 0
    assert on.loop_constants_in_lds == 1
    assert _record(on) == _record(off)


NOT_PLANNED = [
    ("k = 16: 16-lane segments", _row(k=16), None),
    ("k = 22: the constants' area does not fit", _row(k=22), None),
    ("k = 32", _row(k=32), None),
    ("two feet", _row(E=2), None),
    ("fp32", _row(precision=1), None),
    ("raw form", _row(form="raw"), None),
    ("raw form with qf", _row(form="raw_qf"), None),
    ("block costs", _row(form="raw", shape="blocks"), None),
    ("band costs", _row(form="raw", shape="band"), None),
    ("one wave per SIMD: no more waves than SIMDs", _row(B=2048), None),
    ("one wave per SIMD: the switch", _row(knob="two_waves_per_simd", value=0), None),
    ("three problems per wave", _row(B=3072), None),
    ("work stealing", _row(B=6144, num_iters=100), None),
    ("one problem per wave", _row(B=4), None),
]


@pytest.mark.parametrize("what,row,shape", NOT_PLANNED, ids=[c[0] for c in NOT_PLANNED])
def test_not_planned(hiplib, what, row, shape):
    rc, on = _plan(hiplib, row, 1, shape)
    rc0, off = _plan(hiplib, row, 0, shape)
    assert rc == rc0 == 0, what
    assert on.loop_constants_in_lds == 0 and off.loop_constants_in_lds == 0, what
    assert _record(on) == _record(off), what


def test_cone_shape_is_not_planned(hiplib):
    """the exported call plans diagonal, block and band costs only: the cone kernels are a family of their own and it refuses them"""
    rc, out = _plan(hiplib, _row(), 1, shape=3)
    assert rc == _lib.BAD_ARG and out.status == _lib.BAD_ARG and out.loop_constants_in_lds == 0


@pytest.mark.parametrize("k", [16, 17, 21, 22])
def test_mode_0_is_never_and_the_default_is_2(hiplib, k):
    """mode 2, "when it pays", is the default; the measurement (EXPERIMENTS.md) resolved it to "wherever it fits", which is mode 1"""
    assert _plan(hiplib, _row(k=k), 0)[1].loop_constants_in_lds == 0
    assert hiplib.bmpc_set_loop_constants_in_lds(2) == 2
    assert _plan(hiplib, _row(k=k), 2)[1].loop_constants_in_lds == _plan(hiplib, _row(k=k), 1)[1].loop_constants_in_lds == int(17 <= k <= 21)


def test_record_is_the_two_waves_build_s_in_every_mode(hiplib):
    for row in [_row(k=k, B=B) for k in (16, 17, 21, 22, 33) for B in (1, 1025, 4096, 6144)]:
        records = {m: _record(_plan(hiplib, row, m)[1]) for m in (0, 1, 2)}
        assert records[0] == records[1] == records[2], row


def test_fit_function(hiplib):
    """8 (84 + (78 + 2 n) k) bytes per wave at four feet, n = 19 doubles per knot; eight waves share a CU's 160 KB: 20480 bytes each"""
    fits = []
    last = 0
    for k in range(2, 65):
        nbytes = hiplib.bmpc_loop_constants_lds_bytes(4, k - 1)
        assert nbytes == 8 * (84 + (78 + 2 * 19) * k)
        assert nbytes > last      # monotone in k
        last = nbytes
        fit = hiplib.bmpc_loop_constants_fit(4, k - 1)
        assert fit == int(nbytes <= 20480)
        fits.append(fit)
    assert fits == sorted(fits, reverse=True)      # fits up to some k, never beyond it
    assert max(k for k, f in zip(range(2, 65), fits) if f) == 21
    # two feet: records of 33 doubles per knot (the build has no such kernel; the function is the same formula)
    assert hiplib.bmpc_loop_constants_lds_bytes(2, 20) == 8 * (84 + (66 + 2 * 19) * 21)
    assert hiplib.bmpc_loop_constants_lds_bytes(3, 20) == -1 and hiplib.bmpc_loop_constants_lds_bytes(4, 0) == -1
    assert hiplib.bmpc_loop_constants_fit(3, 20) == 0 and hiplib.bmpc_loop_constants_fit(4, 0) == 0
