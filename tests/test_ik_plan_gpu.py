"""The IK launch plan against what a solve does (run with -m gpu): a few solves of tests/golden/ik_dispatch_table.json run again, and
bmpc_ik_batch_t.iters_run and bmpc_ik_last_calcdiff_kernel must agree with the table (recorded on an MI355X before the launch layer was
folded into one plan) and with bmpc_ik_plan_iteration; the solutions must be those of the same batch under default knobs, bit for bit."""
import ctypes as C

import pytest

from bunmpc_amd import _lib
from tests import ik_dispatch_rows as rows

pytestmark = pytest.mark.gpu
SOLVES = {s["name"]: s for s in rows.load()}
NAMES = ("b48_small_knobs", "b48_one_wave", "b48_no_list", "b16_loop", "b5_one_node_pair")
DEFAULT_DIGEST = {}


def default_digest(B, n_col):
    if (B, n_col) not in DEFAULT_DIGEST:
        DEFAULT_DIGEST[(B, n_col)] = rows.IkDeviceBatch(B, n_col, 1).solve()[2]
    return DEFAULT_DIGEST[(B, n_col)]


@pytest.mark.parametrize("name", NAMES)
def test_solve_agrees_with_the_plan_and_the_table(hiplib, name):
    s = SOLVES[name]
    assert s["B"] <= 48 and s["n_col"] <= 5
    iters, last, digest = rows.run(rows.by_name(name))
    assert iters == s["iters_run"] and last == s["last_calcdiff"]
    # the plan of the last look: its derivative kernel is the one the solve launched last
    lk = s["looks"][-1]
    if lk[1] is not None:
        out, sc = _lib.IkIterPlan(), rows.sched_of(s["sched"])
        with rows.knobs({k: v for k, v in s["knobs"].items() if v != rows.DEFAULTS[k]}):
            assert hiplib.bmpc_ik_plan_iteration(s["B"], s["n_col"], s["maxiter"], s["has_list"], s["has_list"], lk[1], C.byref(sc), C.byref(out)) == 0
        assert out.calcdiff.kernel == (b"ik_calcdiff1_kernel" if last else b"ik_calcdiff_kernel")
    assert digest == default_digest(s["B"], s["n_col"])
