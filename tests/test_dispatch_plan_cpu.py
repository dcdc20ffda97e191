"""The dispatch of the centroidal solve as a pure function (bmpc_biconvex_plan_launch) against tests/golden/dispatch_table.json: what
every batch shape of the table was launched as on an MI355X by the commit before the launch layer was folded into one dispatch
(tools/record_dispatch.py wrote the table there, from the "last launch" record of real solves).  No GPU: the function makes no HIP call."""
import ctypes as C

import pytest

from bunmpc_amd import _lib
from tests import dispatch_rows as dr

SIMDS, ROWS = dr.load()


def plan(hiplib, row, simds):
    d, out = dr.descriptor(row), _lib.LaunchPlan()
    with dr.knob(hiplib, row["knob"], row["value"]):
        rc = hiplib.bmpc_biconvex_plan_launch(C.byref(d), dr.SHAPES[row["shape"]], simds, C.byref(out))
    return rc, out


def test_table_covers_what_it_should():
    assert SIMDS == 1024 and len(ROWS) == len(dr.cases())
    assert [tuple(r[c] for c in dr.COLUMNS[:9]) for r in ROWS] == dr.cases()
    seen = lambda col: {r[col] for r in ROWS}
    assert seen("E") >= {2, 4} and seen("k") >= set(dr.K_ALL) and seen("B") >= set(dr.B_ALL) and seen("num_iters") >= {10, 25, 100}
    assert seen("form") == {"harness", "raw", "raw_qf"} and seen("shape") == {"diag", "blocks", "band"} and seen("precision") == {0, 1}
    assert {(r["knob"], r["value"]) for r in ROWS if r["knob"]} == set(dr.KNOBS)
    kernels = seen("kernel")
    assert kernels == {"refused", "biconvex_latency_kernel", "biconvex_admm_kernel", "biconvex_admm_kernel_f32", "biconvex_admm_wg_kernel",
                       "biconvex_admm_steal_kernel", "biconvex_admm_bq_kernel", "biconvex_admm_kq_kernel"}
    assert sum(r["kernel"] == "refused" for r in ROWS) == 12


def test_plan_reproduces_the_recorded_dispatch(hiplib):
    wrong = []
    for i, row in enumerate(ROWS):
        rc, out = plan(hiplib, row, SIMDS)
        if row["kernel"] == "refused":
            ok = rc != 0 and out.status != 0
        else:
            ok = (rc == 0 and out.status == 0 and out.kernel.decode() == row["kernel"] and out.lanes_per_problem == row["lanes"]
                  and out.steal == (row["kernel"] == "biconvex_admm_steal_kernel"))
            if row["kernel"] == "biconvex_latency_kernel":
                ok = ok and out.waves_per_simd == 0      # (the table holds null there: the record after such a launch is the launch before's)
            else:
                ok = ok and out.waves_per_simd == row["waves"]
        if not ok:
            wrong.append((i, row, rc, out.status, out.kernel, out.lanes_per_problem, out.waves_per_simd, out.steal))
    assert not wrong, "%d of %d rows differ, the first: %s" % (len(wrong), len(ROWS), wrong[:5])


def test_knobs_are_restored_and_plan_reads_no_pointer(hiplib):
    """every pointer of the descriptor is null in these calls; the switches are what they were afterwards"""
    names = sorted({n for n, _ in dr.KNOBS})

    def read():
        values = [getattr(hiplib, "bmpc_set_" + n)(0) for n in names]
        for n, v in zip(names, values):
            getattr(hiplib, "bmpc_set_" + n)(v)
        return values
    before = read()
    row = dict(zip(dr.COLUMNS, (4, 21, 6144, "harness", 0, 100, "diag", None, 0)))
    rc, out = plan(hiplib, row, SIMDS)
    assert (rc, out.kernel, out.lanes_per_problem, out.waves_per_simd, out.steal, out.steal_waves) == (0, b"biconvex_admm_steal_kernel", 21, 1, 1, 1024)
    with dr.knob(hiplib, "steal_grid", 512):
        assert plan(hiplib, row, SIMDS)[1].steal_waves == 512
    big = plan(hiplib, row, 2 * SIMDS)[1]      # (2048 waves of three problems: no more than a chip of 2048 SIMDs holds -> no stealing)
    assert (big.kernel, big.lanes_per_problem, big.steal, big.steal_waves) == (b"biconvex_admm_kernel", 21, 0, 0)
    assert read() == before == [1024, 0, 2, 2, 1]


@pytest.mark.parametrize("args", [(None, 0, 1024), ("d", 3, 1024), ("d", -1, 1024), ("d", 0, 0)])
def test_bad_arguments(hiplib, args):
    d, out = dr.descriptor(dict(E=4, k=21, B=4, form="harness", precision=0, num_iters=10)), _lib.LaunchPlan()
    rc = hiplib.bmpc_biconvex_plan_launch(C.byref(d) if args[0] else None, args[1], args[2], C.byref(out))
    assert rc == _lib.BAD_ARG and out.status == _lib.BAD_ARG and out.kernel == b""
    assert hiplib.bmpc_biconvex_plan_launch(C.byref(d), 0, 1024, None) == _lib.BAD_ARG


def test_empty_batch_plans_no_launch(hiplib):
    d, out = dr.descriptor(dict(E=4, k=21, B=0, form="harness", precision=0, num_iters=10)), _lib.LaunchPlan()
    assert hiplib.bmpc_biconvex_plan_launch(C.byref(d), 0, 1024, C.byref(out)) == 0 and out.status == 0 and out.kernel == b""
