"""include/ext/bunmpc_acyclic.h without a GPU: the header against its recorded table and a C compiler, the refusals of its two
calls, and the twin (tests/acyclic_np.py: SoloAcyclicGen driven with recording solver objects) on the synthetic hop table -- that the
cases the GPU tests compare really hold the quirks they are there for."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from bunmpc_amd import _lib, _lib_acyclic, urdf_model
from bunmpc_amd import build as hip_build
from tests import acyclic_np as twin
from tests.test_abi_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_abi  # noqa: E402

ROBOT = os.path.join(ROOT, "bunmpc_amd", "robots", "solo12.json")
EXT = os.path.dirname(_lib_acyclic.HEADER)


@pytest.fixture(scope="module")
def model():
    return urdf_model.RobotModel.from_json(open(ROBOT).read())


@pytest.fixture(scope="module")
def hop(model):
    x, t, t0 = twin.cases()
    return dict(x=x, t=t, t0=t0, a=twin.plan_batch_np(model, twin.hop_plan(), x, t, t0))


def case(t, t0=0.0, state=0):
    return 2 * twin.TIMES.index((t, t0)) + state


# ---- the header -----------------------------------------------------------------------------------------------------------------------

def test_header_equals_its_recorded_table():
    with open(os.path.join(ROOT, "tests", "golden", "abi_acyclic.json")) as f:
        assert record_abi.dump(_lib_acyclic.ABI) == f.read()
    assert sorted(_lib_acyclic.ABI.functions) == ["bmpc_acyclic_plan_batch_device", "bmpc_acyclic_plan_struct_size", "bmpc_hold_batch_device",
                                                  "bmpc_hold_batch_struct_size"]
    assert _lib_acyclic.FRAME_SLOTS == twin.FRAME_SLOTS


def test_header_lives_beside_the_four_and_makes_the_library_stale():
    assert _lib_acyclic.HEADER in hip_build.dependencies() and "bunmpc_acyclic.h" not in _lib.HEADER_NAMES
    assert not set(_lib_acyclic.ABI.functions) & set(_lib._SIGS) and not set(_lib_acyclic.ABI.structs) & set(_lib._ABI.structs)
    jobs = hip_build.compile_jobs()
    assert jobs[-2] == ("acyclic_plan", "acyclic_plan.hip", []) and jobs[-1][0] == "cc_goals"
    lib = _lib_acyclic.lib()      # the symbols are in the library, with the header's struct sizes
    assert lib.bmpc_acyclic_plan_struct_size() == C.sizeof(_lib_acyclic.AcyclicPlan) and lib.bmpc_hold_batch_struct_size() == C.sizeof(_lib_acyclic.HoldBatch)
    assert [f for f, _ in _lib_acyclic.HoldBatch._fields_] == [f for f, _ in _lib.InterpBatch._fields_]      # the shape of bmpc_interp_batch_t


def test_a_c_compiler_lays_the_structs_out_as_ctypes_does(tmp_path):
    cc = _compiler()
    if cc is None:
        pytest.skip("no C compiler on this machine")
    want, lines = [], []
    for cname, cls in _lib_acyclic.ABI.structs.items():
        want.append("%s %d" % (cname, C.sizeof(cls)))
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            want.append("%s.%s %d %d" % (cname, field, getattr(cls, field).offset, getattr(cls, field).size))
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, field, cname, field, cname, field))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bunmpc_acyclic.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", EXT, "-o", str(tmp_path / "layout"), str(src)])
    assert subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")[:-1] == want
    for lang in ("c", "c++"):      # alone, as C and as C++; and it includes nothing
        subprocess.check_call([cc, "-x", lang, "-fsyntax-only", "-Wall", "-Werror", _lib_acyclic.HEADER])
    assert "#include" not in open(_lib_acyclic.HEADER).read()
    both = tmp_path / "both.c"      # and beside the first header
    both.write_text('#include "bunmpc.h"\n#include "ext/bunmpc_acyclic.h"\nint main(void) { return 0; }\n')
    subprocess.check_call([cc, "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.dirname(hip_build.INCLUDE), str(both)])


# ---- refusals: before anything is written or launched, so they need no GPU --------------------------------------------------------------

_ARRAYS = ("x", "t", "t0", "dt_arr", "tab_cnt_plan", "tab_X_nom", "tab_X_ter", "tab_bounds", "tab_swing_wt", "tab_state_reg", "tab_state_wt",
           "tab_state_scale", "tab_ctrl_wt", "tab_ctrl_scale", "cnt_plan", "dt", "dt_ik", "x_init", "X_nom", "X_ter", "bounds", "ik_tasks", "state_w",
           "x_reg", "ctrl_w", "status")


def _plan_desc(dm, **kw):
    """a descriptor that passes every check (its arrays are never touched: every call below is refused), with fields replaced"""
    d = _lib_acyclic.AcyclicPlan()
    d.B, d.n_col, d.model = 3, 12, dm.h
    d.n_cnt, d.n_x, d.n_b, d.n_sw, d.n_s, d.n_c = 3, 3, 2, 1, 2, 2
    for j, name in enumerate(("FL_FOOT", "FR_FOOT", "HL_FOOT", "HR_FOOT")):
        d.foot_frame[j] = dm.model.frame_id(name)
    d.cnt_wt, d.cent_wt[0], d.cent_wt[1], d.state_end = 1e3, 0.1, 50.0, 0.9
    for name in _ARRAYS:
        setattr(d, name, 4096)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,word", [(dict(B=-1), "B"), (dict(n_col=0), "n_col"), (dict(n_col=256), "n_col"), (dict(model=None), "model")] +
                         [({n: bad}, n) for n in ("n_cnt", "n_x", "n_b", "n_s", "n_c") for bad in (0, 17)] + [(dict(n_sw=-1), "n_sw"), (dict(n_sw=17), "n_sw")] +
                         [(dict(foot_frame=(2, -1)), "foot_frame[2]"), (dict(foot_frame=(0, 100000)), "foot_frame[0]"),
                          (dict(cnt_wt=float("nan")), "cnt_wt"), (dict(cnt_wt=float("inf")), "cnt_wt"), (dict(cent_wt=(1, float("nan"))), "cent_wt"),
                          (dict(cent_wt=(0, float("-inf"))), "cent_wt"), (dict(state_end=float("nan")), "state_end")] +
                         [({n: None}, n) for n in _ARRAYS])
def test_plan_refusals_name_the_field(model, kw, word):
    from bunmpc_amd.inverse_kinematics_cpp import as_device_model
    dm = as_device_model(model)
    rc = _lib_acyclic.lib().bmpc_acyclic_plan_batch_device(C.byref(_plan_desc(dm, **kw)), None)
    assert rc == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()


def test_plan_accepts_no_swing_table_when_there_are_no_swing_rows(model):
    """n_sw = 0: tab_swing_wt is not looked at -- the next check (a foot frame) is what refuses this descriptor"""
    from bunmpc_amd.inverse_kinematics_cpp import as_device_model
    dm = as_device_model(model)
    lib = _lib_acyclic.lib()
    assert lib.bmpc_acyclic_plan_batch_device(None, None) == _lib.BAD_ARG and "null plan descriptor" in _lib.last_error()
    rc = lib.bmpc_acyclic_plan_batch_device(C.byref(_plan_desc(dm, n_sw=0, tab_swing_wt=None, foot_frame=(3, -5))), None)
    assert rc == _lib.BAD_ARG and "foot_frame[3]" in _lib.last_error()


def _hold_desc(**kw):
    d = _lib_acyclic.HoldBatch()
    d.B, d.n_knots, d.width, d.size, d.max_rows, d.dt_stride, d.step = 2, 13, 37, 12, 600, 12, 0.001
    d.knots = d.dt = d.out = d.rows = 4096
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,word", [(dict(B=-1), "B"), (dict(n_knots=0), "n_knots"), (dict(width=0), "width"), (dict(size=0), "size"), (dict(max_rows=0), "max_rows"),
                                     (dict(size=14), "size"), (dict(dt_stride=11), "dt_stride"), (dict(step=0.0), "step"), (dict(step=float("nan")), "step"),
                                     (dict(B=1 << 30, max_rows=1 << 20), "2^38")] + [({n: None}, n) for n in ("knots", "dt", "out", "rows")])
def test_hold_refusals_name_the_field(kw, word):
    lib = _lib_acyclic.lib()
    rc = lib.bmpc_hold_batch_device(C.byref(_hold_desc(**kw)), None)
    assert rc == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()
    assert lib.bmpc_hold_batch_device(None, None) == _lib.BAD_ARG


# ---- the twin on the hop table ----------------------------------------------------------------------------------------------------------

def test_first_knot_rule(hop):
    dt = hop["a"]["dt"]
    assert dt[case(0.02), 0] == 0.05 - 0.02 and dt[case(0.27), 0] == 0.05 - 0.02 and dt[case(0.88), 0] == 0.05 - 0.03      # shortened: 0.03, 0.02
    assert abs(dt[case(0.02), 0] - 0.03) < 1e-15 and abs(dt[case(0.88), 0] - 0.02) < 1e-15
    assert np.round(np.remainder(0.6, 0.05), 2) == 0.05 and dt[case(0.6), 0] == 0.05                                     # dt == 0 becomes dt_arr[0]
    assert np.all(dt[:, 1:] == 0.05) and np.all(hop["a"]["dt_ik"] == 0.05)                                               # the IK stage sees no rule
    # t0 != 0, absolute t off the grid: the rule is on t (0.37 -> 0.03), not on t - t0 (0.15 -> 0.05)
    assert abs(dt[case(0.37, 0.22), 0] - 0.03) < 1e-15 and np.round(np.remainder(0.37 - 0.22, 0.05), 2) in (0.0, 0.05)


def test_the_two_time_walks_disagree_at_knot_10(hop):
    """t = t0: the contact walk's unrounded sum stays below 0.5 at knot 10 (flight), the cost tables' rounded walk is at 0.5 (landing)"""
    a, b = hop["a"], case(0.0)
    assert np.all(a["cnt_plan"][b, 10, :, 0] == 0.0) and np.all(a["cnt_plan"][b, 11, :, 0] == 1.0)
    assert np.array_equal(a["X_nom"][b, 90:99], twin.hop_plan().X_nom[2][:9]) and np.array_equal(a["bounds"][b, 10], twin.hop_plan().bounds[1][:6])
    assert a["ik_tasks"][b, 10, 31] == 4e-2 and a["ik_tasks"][b, 9, 31] == 1e-2 and a["ik_tasks"][b, 10, 32] == 3e-2 and a["ik_tasks"][b, 9, 32] == 1e-2
    assert np.all(a["ik_tasks"][b, 10, 0:20:5] == 0.0)      # no contact task in the flight, and the swing window is over


def test_phases_tasks_and_the_running_control_weight(hop):
    a, p = hop["a"], twin.hop_plan()
    b = case(0.05)
    # (knot 9, motion time 0.5, is still in the flight for the contact walk: its unrounded sum stays below 0.5)
    assert np.all(a["cnt_plan"][b, :5, :, 0] == 1.0) and np.all(a["cnt_plan"][b, 5:10, :, 0] == 0.0) and np.all(a["cnt_plan"][b, 10:, :, 0] == 1.0)
    assert np.allclose(a["cnt_plan"][b, 10, :, 1] - a["cnt_plan"][b, 0, :, 1], 0.05, atol=1e-15)                     # landing 5 cm ahead
    assert np.all(a["ik_tasks"][b, 0, 0:20:5] == p.cnt_wt)                                                           # four contact tasks
    swing = [i for i in range(12) if np.any(a["ik_tasks"][b, i, 0:20:5] == 4e2)]
    assert swing == [6, 7] and np.all(a["ik_tasks"][b, 6, 4:20:5] == 0.09)                                           # the window, inside the flight
    assert a["ik_tasks"][b, 12, 32] == 3e-4 and a["ik_tasks"][b, 0, 32] == p.ctrl_wt[0][0] != p.ctrl_scale[0][0]     # ctrl_wt[k][0] runs, the scale ends
    assert np.all(a["ik_tasks"][b, :, 20] == p.cent_wt[0]) and np.all(a["ik_tasks"][b, :, 24] == p.cent_wt[1])
    assert np.array_equal(a["X_nom"][b, 0:9], a["x_init"][b]) and np.all(a["status"] == 0) and a["frames"].max() == 4
    assert np.array_equal(a["x_reg"][b, 0], p.state_reg[0][:37]) and np.array_equal(a["x_reg"][b, 12], p.state_reg[1][:37])
    assert not np.array_equal(a["x_init"][b], a["x_init"][b + 1]) and np.array_equal(a["bounds"][b], a["bounds"][b + 1])      # the perturbed state


def test_last_rows_are_held_past_the_end(hop):
    a, p = hop["a"], twin.hop_plan()
    for t in (0.95, 1.5):
        b = case(t)
        assert np.array_equal(a["cnt_plan"][b], np.tile(np.array(p.cnt_plan[-1])[:, :4], (12, 1, 1)))
        assert np.array_equal(a["bounds"][b], np.tile(p.bounds[-1][:6], (12, 1))) and np.array_equal(a["X_ter"][b], p.X_ter)
        assert np.array_equal(a["X_nom"][b, 9:], np.tile(p.X_ter, 11)) and np.all(a["ik_tasks"][b, :, 31] == 4e-2)
        assert np.all(a["ik_tasks"][b, :12, 32] == 3e-2) and np.array_equal(a["ctrl_w"][b], np.tile(p.ctrl_wt[1][:18], (12, 1)))
    b = case(0.6)      # the end is reached inside the horizon: the terminal reference is the table's X_ter, knots before it the last row
    assert np.array_equal(a["X_ter"][b], p.X_ter) and np.array_equal(a["X_nom"][b, 9:18], p.X_nom[2][:9])
    b = case(0.3)      # ... and not reached: the last knot's own row
    assert np.array_equal(a["X_ter"][b], p.X_nom[2][:9])


def test_nodes_before_the_motion_have_no_costs(hop):
    """t - t0 = -0.1: knots 0 and 1 (motion times -0.1, -0.05) match no interval"""
    a, b = hop["a"], case(-0.1)
    assert np.all(a["ik_tasks"][b, :2, 31] == 0) and np.all(a["ik_tasks"][b, :2, 32] == 0) and np.all(a["ik_tasks"][b, 2:, 31] != 0)
    assert np.all(a["state_w"][b, :2] == 0) and np.all(a["ctrl_w"][b, :2] == 0) and np.all(a["bounds"][b, :2] == 0) and np.all(a["cnt_plan"][b, :2] == 0)
    neutral = np.zeros(37)
    neutral[6] = 1.0
    assert np.array_equal(a["x_reg"][b, 0], neutral) and np.all(a["X_nom"][b, 9:18] == 0) and np.all(a["ik_tasks"][b, :2, 0:20:5] == 0)


def test_a_foot_in_contact_and_swinging_overflows_the_slots(model):
    x, t, t0 = twin.cases()
    a = twin.plan_batch_np(model, twin.slot_plan(), x[:6], t[:6], t0[:6])
    assert a["frames"].max() == 5 and np.all(a["status"] == twin.FRAME_SLOTS)
    b, i = 0, int(np.argmax(a["frames"][0]))
    assert np.all(a["ik_tasks"][b, i, 0:20:5] == 1.2e3)      # the four contact tasks are kept, in order; the swing task is the one dropped


def test_hold_np_is_the_mirrors_expansion():
    knots = np.arange(3 * 4, dtype=float).reshape(3, 4)
    out = twin.hold_np(knots, [0.003, 0.0, 0.002], 3)
    assert np.array_equal(out, knots[[0, 0, 0, 2, 2]]) and np.array_equal(twin.hold_np(knots, [0.003, 0.0, 0.002], 3, max_rows=4), out[:4])
