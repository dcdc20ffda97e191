"""The launch plan of the IK-DDP loop as a pure function (bmpc_ik_plan_iteration: plan_batch + plan_iteration of
bunmpc_amd/csrc/ik_plan.h) against tests/golden/ik_dispatch_table.json: what every host look of the table's solves launched on an
MI355X on the commit before the launch layer was folded into one plan (tools/record_ik_dispatch.py wrote the table there, from kernel
traces of real solves).  No GPU: the function makes no HIP call."""
import ctypes as C

import pytest

from bunmpc_amd import _lib
from tests import ik_dispatch_rows as rows

SOLVES = rows.load()
STAGES = ("state", "calcdiff", "backward", "forward")


def plan(hiplib, s, active, sched=None):
    out = _lib.IkIterPlan()
    sc = rows.sched_of(s["sched"] if sched is None else sched)
    rc = hiplib.bmpc_ik_plan_iteration(s["B"], s["n_col"], s["maxiter"], s["has_list"], s["has_list"], active, C.byref(sc), C.byref(out))
    assert rc == 0 and out.status == 0, _lib.last_error()
    return out


def table_knobs(s):
    return {k: v for k, v in s["knobs"].items() if v != rows.DEFAULTS[k]}


def look_of(out):
    return [out.chunk] + [[getattr(out, st).kernel.decode(), getattr(out, st).grid, getattr(out, st).block] for st in STAGES]


def test_table_is_the_one_the_tool_records():
    assert [(s["name"], s["B"], s["n_col"], s["has_list"], table_knobs(s), {k: v for k, v in s["sched"].items() if v}) for s in SOLVES] == \
        [tuple(s) for s in rows.solves()]
    assert all(s["maxiter"] == rows.MAXITER for s in SOLVES)


def test_table_covers_what_it_should(hiplib):
    looks = [(s, lk) for s in SOLVES for lk in s["looks"]]
    # the five line-search mappings, told apart by kernel and grid over the n problems of the Riccati grid (sizes where two readings
    # coincide left out): <1> on ceil(n / 4) and on n workgroups, <2> and <3> on n + the wide list's 64, <3> on 3 n

    def shape(g, n):
        return "n/4" if g == (n + 3) // 4 and n > 1 else "n" if g == n and n > 1 else "3n" if g == 3 * n != n + 64 else "n+64" if g == n + 64 != 3 * n else "?"
    grids = {(lk[6][0], shape(lk[6][1], lk[5][1])) for s, lk in looks if s["has_list"]}
    assert grids >= {("ik_forward_kernel<1>", "n/4"), ("ik_forward_kernel<1>", "n"), ("ik_forward_kernel<2>", "n+64"), ("ik_forward_kernel<3>", "n+64"),
                     ("ik_forward_kernel<3>", "3n")}
    assert {lk[5][0] for _, lk in looks} == {"ik_backward_kernel<1>", "ik_backward_kernel<2>"}
    assert {lk[4][0] for _, lk in looks} == {"ik_calcdiff_kernel", "ik_calcdiff1_kernel"}
    out = plan(hiplib, SOLVES[0], 1)
    assert {lk[2] for _, lk in looks} >= {1, out.tail_chunk} and out.tail_chunk == 3
    assert any(s["fused_direct"] for s in SOLVES) and any(s["express_launches"] for s in SOLVES) and any(not s["has_list"] and s["looks"] for s in SOLVES)
    # the refusals: a horizon above the fused kernel's, with a batch small enough for fused-direct and one forced into the express lane
    assert out.max_fused_col == 63
    long_ = [s for s in SOLVES if s["n_col"] > out.max_fused_col]
    assert any(s["B"] <= 16 for s in long_) and any(s["B"] >= 64 and s["sched"]["debug_inject"] == 2 for s in long_)
    assert all(not s["fused_direct"] and not s["express_launches"] for s in long_)
    # geometry: one node pair, three nodes, a part-filled wave of the four-per-wave line search, an odd pair count on the one-wave kernel
    assert {1, 2} <= {s["n_col"] for s in SOLVES}
    assert any(lk[6][:2] == ["ik_forward_kernel<1>", 2] and lk[5][1] == 5 for _, lk in looks)
    assert any(lk[4][0] == "ik_calcdiff1_kernel" and (lk[5][1] * ((s["n_col"] + 2) // 2)) % 2 == 1 for s, lk in looks)


class hiplib_knobs:
    """the library with a solve's knobs set for one call each (the table's solves ran under them)"""

    def __init__(self, lib, s):
        self.lib, self.values = lib, table_knobs(s)

    def bmpc_ik_plan_iteration(self, *args):
        with rows.knobs(self.values):
            return self.lib.bmpc_ik_plan_iteration(*args)


@pytest.mark.parametrize("s", SOLVES, ids=[s["name"] for s in SOLVES])
def test_plan_reproduces_the_recorded_launches(hiplib, s):
    lib = hiplib_knobs(hiplib, s)
    b = plan(lib, s, s["B"])
    assert b.fused_direct == s["fused_direct"] and (not s["fused_direct"] or b.fused_grid == s["fused_grid"])
    if s["fused_direct"]:
        assert s["looks"] == [] and s["express_launches"] == 0
        return
    assert (b.express_cap > 0) == (s["express_launches"] > 0) and (not s["express_launches"] or b.express_grid == s["express_grid"])
    if s["express_launches"]:     # the lane's look runs in front of iterations first .. last until a host look has seen it take its problems
        assert 1 <= s["select_launches"] == s["express_launches"] <= b.express_last_iter - b.express_first_iter + 1
    it, wrong = 0, []
    for lk in s["looks"]:
        first, active, chunk = lk[:3]
        assert first == it
        want = [chunk] + lk[3:]
        candidates = [active] if active is not None else range(1, s["B"] + 1)     # (no active list: the grids do not show the look)
        got = []
        for a in candidates:
            out = plan(lib, s, a)
            got = look_of(out)
            got[0] = min(got[0], s["maxiter"] - it)       # (the loop enqueues no iteration past maxiter)
            if got == want:
                assert active is None or out.n_launch == active
                break
        else:
            wrong.append((lk, got))
        it += chunk
    assert not wrong, "%d of %d looks differ, the first: %s" % (len(wrong), len(s["looks"]), wrong[:3])
    assert s["iters_run"] <= it <= s["maxiter"]
    assert s["last_calcdiff"] == (s["looks"][-1][4][0] == "ik_calcdiff1_kernel")


BASE = dict(B=48, n_col=5, maxiter=40, has_list=1)


def test_sched_overrides_field_by_field(hiplib):
    """bmpc_ik_sched_t through resolve_knobs: 0 = the process default, < 0 = never, n > 0 = n"""
    with rows.knobs(dict(spec_below=48, all_steps=48, gains_wave_below=48, express_cap=7, fused_direct=0)):
        s64 = dict(BASE, B=64)
        # spec_below: default 48 -> side by side at 48; never -> four per wave, one iteration per look; 10 -> only at <= 10
        with rows.knobs(dict(all_steps=0)):
            assert (plan(hiplib, BASE, 48, {}).fwd_map, plan(hiplib, BASE, 48, {}).chunk) == (2, 3)
            assert (plan(hiplib, BASE, 48, dict(spec_below=-1)).fwd_map, plan(hiplib, BASE, 1, dict(spec_below=-1)).chunk) == (0, 1)
            assert [plan(hiplib, BASE, a, dict(spec_below=10)).fwd_map for a in (11, 10, 4, 3)] == [0, 2, 2, 3]
        # all_steps_below
        assert plan(hiplib, BASE, 48, {}).fwd_map == 4
        assert plan(hiplib, BASE, 1, dict(all_steps_below=-1)).fwd_map == 3
        assert [plan(hiplib, BASE, a, dict(all_steps_below=5)).fwd_map for a in (6, 5)] == [3, 4]
        # gains_wave_below
        assert plan(hiplib, BASE, 48, {}).bwd_waves == 2
        assert plan(hiplib, BASE, 1, dict(gains_wave_below=-1)).bwd_waves == 1
        assert [plan(hiplib, BASE, a, dict(gains_wave_below=20)).bwd_waves for a in (21, 20)] == [1, 2]
        # express_cap (not a threshold: the lane's capacity)
        assert plan(hiplib, s64, 64, {}).express_cap == 7
        assert plan(hiplib, s64, 64, dict(express_cap=-1)).express_cap == 0
        assert (plan(hiplib, s64, 64, dict(express_cap=300)).express_cap, plan(hiplib, s64, 64, dict(express_cap=300)).express_grid) == (300, 256)
        assert plan(hiplib, BASE, 48, dict(express_cap=9)).express_cap == 0        # (fewer than 64 problems: no lane)
        # debug_inject is no knob of the plan
        assert look_of(plan(hiplib, BASE, 48, dict(debug_inject=2))) == look_of(plan(hiplib, BASE, 48, {}))


SETTERS = [("speculative_below", 1024, 30, lambda p: p.chunk, 48, (3, 1)),      # (name, default, value, what shows it, active, (before, after)): 48 > 30
           ("spec_one_wave_above", 0, 20, lambda p: p.fwd_map, 48, (2, 1)),
           ("all_steps", 0, 48, lambda p: p.fwd_map, 48, (2, 4)),
           ("gains_wave_below", 512, 47, lambda p: p.bwd_waves, 48, (2, 1)),
           ("calcdiff_one_wave_above", 1024, 143, lambda p: p.calcdiff.kernel, 48, (b"ik_calcdiff_kernel", b"ik_calcdiff1_kernel")),
           ("express_capacity", 96, 5, lambda p: p.express_grid, 64, (96, 5)),
           ("fused_direct_max", 16, 48, lambda p: p.fused_direct, 48, (0, 1))]


@pytest.mark.parametrize("name,default,value,show,active,expect", SETTERS, ids=[s[0] for s in SETTERS])
def test_setters_return_the_old_value_and_show_in_the_next_plan(hiplib, name, default, value, show, active, expect):
    fn = getattr(hiplib, "bmpc_ik_set_" + name)
    s = dict(BASE, B=active)
    with rows.knobs(dict(spec_below=48) if name != "speculative_below" else {}):
        assert show(plan(hiplib, s, active, {})) == expect[0]
        assert fn(value) == default
        try:
            assert show(plan(hiplib, s, active, {})) == expect[1]
        finally:
            assert fn(default) == value
        assert show(plan(hiplib, s, active, {})) == expect[0]


def test_setters_that_the_plan_does_not_show(hiplib):
    assert hiplib.bmpc_ik_set_blocking_waits(0) == 1 and hiplib.bmpc_ik_set_blocking_waits(5) == 0 and hiplib.bmpc_ik_set_blocking_waits(1) == 1
    assert hiplib.bmpc_ik_set_express_near(0.25) == 1.0 and hiplib.bmpc_ik_set_express_near(1.0) == 0.25


@pytest.mark.parametrize("args", [(0, 5, 40, 1), (4, 0, 40, 1), (4, 256, 40, 1), (4, 5, 0, 1), (4, 5, 40, 0), (4, 5, 40, 5)])
def test_bad_arguments(hiplib, args):
    out = _lib.IkIterPlan()
    B, n_col, maxiter, active = args
    assert hiplib.bmpc_ik_plan_iteration(B, n_col, maxiter, 1, 1, active, None, C.byref(out)) == _lib.BAD_ARG and out.status == _lib.BAD_ARG
    assert hiplib.bmpc_ik_plan_iteration(4, 5, 40, 1, 1, 4, None, None) == _lib.BAD_ARG
