"""Turning commands without a GPU: the third header (include/bunmpc_turn.h) against its recorded table,
problems.make_wb_batch(w_des=...) against the single-problem harness (bunmpc_amd/cyclic_gen.py :: SoloMpcGaitGen, which restates
abstract_cyclic_gen.py) problem by problem, a hand-checked pure-yaw state, and the refusals of the two C calls (they come before the
first HIP call)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from bunmpc_amd import _lib, problems
from bunmpc_amd.plan_batch import turn_struct
from bunmpc_amd import build as hip_build
from tests import turn_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_abi  # noqa: E402

PLAN = ("cnt_plan", "swing_time", "dt", "x_init", "X_nom", "X_ter")


# ---- 1. the third header -----------------------------------------------------------------------------------------------------------------

def test_turn_header_equals_its_recorded_table():
    """tests/golden/abi_turn.json: tools/record_abi.py's table of include/bunmpc_turn.h; a change of the header is re-recorded and
    reviewed as a diff of the file"""
    with open(os.path.join(ROOT, "tests", "golden", "abi_turn.json")) as f:
        golden = f.read()
    assert record_abi.dump(_lib.HEADERS["bunmpc_turn.h"]) == golden
    table = json.loads(golden)
    assert sorted(table["functions"]) == ["bmpc_plan_batch_turn_device", "bmpc_turn_struct_size", "bmpc_wb_plan_batch_turn_device"]
    assert sorted(table["structs"]) == ["bmpc_turn_t"]
    for name in ("bmpc_plan_batch_turn_device", "bmpc_wb_plan_batch_turn_device"):
        assert _lib.HEADERS["bunmpc_turn.h"].functions[name] == (C.c_int, [C.c_void_p] * 5)


def test_the_first_two_headers_are_untouched_by_the_third():
    turn, first, goals = (_lib.HEADERS[h] for h in ("bunmpc_turn.h", "bunmpc.h", "bunmpc_goals.h"))
    assert len(first.functions) == 164 and len(first.structs) == 18 and len(goals.functions) == 5
    assert _lib.Turn is turn.structs["bmpc_turn_t"] and "bmpc_turn_t" not in first.structs and "bmpc_turn_t" not in goals.structs
    assert not set(turn.functions) & (set(first.functions) | set(goals.functions))
    assert os.path.join(os.path.dirname(hip_build.INCLUDE), "bunmpc_turn.h") in hip_build.dependencies()
    lib = _lib.lib()                                         # every declared symbol is in the library, and the struct has its size
    assert lib.bmpc_turn_struct_size() == C.sizeof(_lib.Turn) == 16


# ---- 2. the numpy builder against the single-problem harness --------------------------------------------------------------------------------

def test_the_seed_is_away_from_rounding_ties():
    assert turn_np.assert_away_from_ties(turn_np.batch("trot").x) > 1e-5


@pytest.mark.parametrize("terrain", [False, True])
@pytest.mark.parametrize("gait", ["trot", "trot_turn"])
def test_rows_without_a_command_are_the_batch_without_commands(gait, terrain):
    """w == 0 rows of the mixed batch: array_equal on every array; and w_des = zeros is w_des = None"""
    wb, plain = turn_np.batch(gait, True, terrain), turn_np.batch(gait, False, terrain)
    still = turn_np.W_DES == 0
    assert still.sum() == 2 and np.array_equal(wb.x, plain.x)
    for k in PLAN:
        a, b = getattr(wb.dyn, k), getattr(plain.dyn, k)
        assert np.array_equal(a[still], b[still]), k
    assert np.array_equal(wb.ik_tasks[still], plain.ik_tasks[still]) and np.array_equal(wb.x_reg, plain.x_reg)
    assert np.array_equal(wb.state_w, plain.state_w) and np.array_equal(wb.ctrl_w, plain.ctrl_w)
    # ... and the commands move the others: steps, orientation correction, yaw momentum
    for k in ("cnt_plan", "X_nom", "X_ter"):
        assert all(not np.array_equal(getattr(wb.dyn, k)[b], getattr(plain.dyn, k)[b]) for b in np.nonzero(~still)[0]), k
    g, ik = turn_np.GAITS[gait]
    zeros = problems.make_wb_batch(turn_np.model(), turn_np.B, seed=turn_np.SEED, gait=g, ik=ik, w_des=np.zeros(turn_np.B),
                                   height_map=turn_np.stairs() if terrain else None)
    for k in PLAN:
        assert np.array_equal(getattr(zeros.dyn, k), getattr(plain.dyn, k)), k
    assert np.array_equal(zeros.ik_tasks, plain.ik_tasks)


@pytest.mark.parametrize("terrain", [False, True])
@pytest.mark.parametrize("gait", ["trot", "trot_turn"])
def test_every_row_equals_the_harness(monkeypatch, gait, terrain):
    """make_wb_batch(w_des=W_DES), row by row (the rows without a command too), against SoloMpcGaitGen.create_cnt_plan / create_costs
    with recorders for solver handles: the comparison of tests/test_harness_gpu.py::test_one_mpc_call_equals_the_batch_row; and the
    yaw-momentum reference is yaw_inertia * w exactly"""
    wb = turn_np.batch(gait, True, terrain)
    Izz, m = turn_np.yaw_inertia(), wb.dyn.meta
    assert m["yaw_inertia"] == Izz and np.array_equal(m["w_des"], turn_np.W_DES)
    for i, w in enumerate(turn_np.W_DES):
        gg = turn_np.host_plan(monkeypatch, gait, wb.x[i, :19], wb.x[i, 19:], m["t0"][i], m["v_des_body"][i], w,
                               height_map=turn_np.stairs() if terrain else None)
        assert np.allclose(gg.cnt_plan, wb.dyn.cnt_plan[i], rtol=0, atol=1e-15) and np.array_equal(gg.dt_arr, wb.dyn.dt[i]), i
        assert np.array_equal(gg.swing_time, wb.dyn.swing_time[i]), i
        assert np.allclose(gg.X_nom, wb.dyn.X_nom[i], rtol=0, atol=1e-15) and np.allclose(gg.X_ter, wb.dyn.X_ter[i], rtol=0, atol=1e-15), i
        if w != 0:
            assert np.all(wb.dyn.X_nom[i, 8::9] == Izz * w) and wb.dyn.X_ter[i, 8] == wb.dyn.X_nom[i, 8], i
            assert np.all(gg.X_nom[8::9] == Izz * w) and gg.X_ter[8] == Izz * w, i      # (I [0, 0, w])[2] is that product
        # the IK tasks the harness hands to its solver are the batch's task blocks
        tasks = [a for name, a in gg.ik.calls if name == "add_position_tracking_task_single"]
        blocks = wb.ik_tasks[i, :wb.ik_T, :20].reshape(wb.ik_T, 4, 5)
        assert len(tasks) == np.count_nonzero(blocks[..., 0])
        for frame, pos, wt, name, node in tasks:
            j = wb.frame_ids.index(frame)
            assert blocks[node, j, 0] == wt and np.allclose(blocks[node, j, 2:5], pos, rtol=0, atol=1e-15), (i, node, j)


# ---- 3. a pure yaw, by hand -----------------------------------------------------------------------------------------------------------------

def test_pure_yaw_by_hand():
    """A base turned by yaw about z and nothing else: R_q = Rz(yaw).  With a command R_des = Rz(yaw) too, so amom = log3(I) = 0 and
    X_nom[6::9], X_nom[7::9], X_ter[6:8] vanish (to 1e-15), with the yaw momentum yaw_inertia * w behind them; without one R_des = I,
    amom = log3(Rz(-yaw)) = (0, 0, -yaw): the two branches cannot be taken for one another."""
    yaw, w = 0.7, 0.4
    q = np.tile(problems.SOLO12_Q0, (2, 1))
    q[:, 3:7] = [0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)]
    args = (turn_np.model(), q, np.zeros((2, 18)), np.zeros(2), np.array([[0.2, 0.0, 0.0]] * 2))
    wb = problems.wb_batch_of_states(*args, w_des=np.array([w, 0.0]))
    H, Izz, oc = wb.dyn.H, turn_np.yaw_inertia(), problems.TROT.ori_correction
    Xn, Xt = wb.dyn.X_nom.reshape(2, H, 9), wb.dyn.X_ter
    assert np.abs(Xn[0, :, 6:8]).max() <= 1e-15 and np.abs(Xt[0, 6:8]).max() <= 1e-15
    assert np.all(Xn[0, :, 8] == Izz * w) and Xt[0, 8] == Izz * w and 0.01 < Izz < 0.1      # Solo12: 2.5 kg, ~0.2 m from the axis
    assert np.abs(Xt[1, 6:9] - [0.0, 0.0, -yaw]).max() <= 1e-15
    assert np.abs(Xn[1, :, 6:9] - [0.0, 0.0, -yaw * oc[2]]).max() <= 1e-15
    # the desired velocity turns with the base (:642-643) and the steps bend (:285-286): the foot locations differ between the rows
    assert np.allclose(Xn[:, :, 3:5], 0.2 * np.array([np.cos(yaw), np.sin(yaw)]), rtol=0, atol=1e-15)
    assert np.abs(wb.dyn.cnt_plan[0, :, :, 1:3] - wb.dyn.cnt_plan[1, :, :, 1:3]).max() > 1e-3


def test_turning_trot_has_the_references_numbers():
    """motions/cyclic/solo12_trot.py:46-74"""
    g, ik = problems.TROT_TURN, problems.TROT_TURN_IK
    assert g.phase_offset == (0.0, 0.4, 0.4, 0.0) and g.gait_horizon == 1.0 and g.step_ht == 0.05 and g.ori_correction == (0.0, 0.5, 0.4)
    assert g.horizon == 10 and turn_np.batch("trot_turn").ik_T == 5
    assert (g.gait_period, g.stance_percent, g.gait_dt, g.nom_ht, g.rho) == (0.5, (0.6,) * 4, 0.05, 0.2, 5e4)
    for k in ("W_X", "W_X_ter", "W_F"):
        assert np.array_equal(getattr(g, k), getattr(problems.TROT, k))
    differ = np.nonzero(ik["state_wt"] != problems.TROT_IK["state_wt"])[0]
    assert list(differ) == [5, 23] and ik["state_wt"][5] == 10 and ik["state_wt"][23] == 10
    assert all(np.array_equal(ik[k], problems.TROT_IK[k]) for k in ("ctrl_wt", "swing_wt", "cent_wt", "reg_wt"))
    from bunmpc_amd import dataset
    assert dataset.GAIT_VALUE.get(g.name, 0.0) == dataset.GAIT_VALUE.get("a gait nobody has heard of", 0.0)


# ---- 4. refusals through the C calls, no GPU ----------------------------------------------------------------------------------------------------

def _plan_desc(keep, **kw):
    d = _lib.PlanBatch()
    d.B, d.n_col, d.n_gaits = 2, 4, 1
    buf = np.zeros(1024)
    keep.append(buf)
    for k in ("gaits", "t0", "com", "feet0", "v_des", "w_des", "x_init", "cnt_plan", "swing_time", "dt", "X_nom", "X_ter"):
        setattr(d, k, buf.ctypes.data)      # host memory: a refused call reads no array
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _wb_desc(keep, **kw):
    from bunmpc_amd.inverse_kinematics_cpp import as_device_model
    dm = as_device_model(turn_np.model())
    d = _lib.WbPlanBatch()
    d.B, d.n_col, d.ik_col, d.model = 2, 4, 2, dm.h
    buf = np.zeros(4096)
    keep.extend([dm, buf])
    for name in ("gait", "x", "t0", "v_des_body", "com", "feet0", "v_des", "w_des", "hip_off", "amom", "x_init", "cnt_plan", "swing_time", "dt",
                 "X_nom", "X_ter", "ik_tasks"):
        setattr(d, name, buf.ctypes.data)
    for j in range(4):
        d.foot_frame[j] = dm.model.frame_id(problems.FEET[j])
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _terrain_desc(keep, **kw):
    Z = np.zeros((8, 8))
    keep.append(Z)
    t = _lib.Terrain(nx=8, ny=8, x0=0.0, y0=0.0, cell=0.1, heights=Z.ctypes.data, sheights=0)
    for k, v in kw.items():
        setattr(t, k, v)
    return t


BAD_INERTIA = [0.0, -0.05, float("nan"), float("inf"), -float("inf")]


def test_refusals_of_the_centroidal_level_call():
    keep = []
    call = _lib.lib().bmpc_plan_batch_turn_device
    d, t = _plan_desc(keep), _terrain_desc(keep)
    w = np.zeros(2)
    for terrain in (None, C.byref(t)):
        for bad in BAD_INERTIA:
            assert call(C.byref(d), terrain, None, C.byref(_lib.Turn(None, bad)), None) == _lib.BAD_ARG, bad
            assert "yaw_inertia" in _lib.last_error(), _lib.last_error()
        assert call(C.byref(d), terrain, None, C.byref(_lib.Turn(w.ctypes.data, 0.05)), None) == _lib.BAD_ARG
        assert "bmpc_turn_t.w_des must be NULL" in _lib.last_error(), _lib.last_error()
    turn = C.byref(_lib.Turn(None, 0.05))
    # everything the plain calls refuse, with their messages; with a turn and without (turn == NULL is the plain call)
    for tn in (turn, None):
        assert call(None, None, None, tn, None) == _lib.BAD_ARG and "null plan descriptor" in _lib.last_error()
        for field, value, word in (("n_col", 0, "n_col < 1"), ("B", -1, "B < 0"), ("gaits", None, "gait"), ("n_gaits", 2, "gait_id"), ("t0", None, "input"),
                                   ("w_des", None, "input"), ("cnt_plan", None, "output")):
            assert call(C.byref(_plan_desc(keep, **{field: value})), None, None, tn, None) == _lib.BAD_ARG and word in _lib.last_error(), field
        for kw, word in ((dict(heights=None), "heights"), (dict(nx=1), "[2, 4096]"), (dict(cell=0.0), "cell"), (dict(sheights=63), "sheights")):
            assert call(C.byref(d), C.byref(_terrain_desc(keep, **kw)), None, tn, None) == _lib.BAD_ARG and word in _lib.last_error(), kw
    # B == 0: nothing to do -- but a bad turn is still refused
    empty = _plan_desc(keep, B=0)
    assert call(C.byref(empty), None, None, turn, None) == _lib.OK and call(C.byref(empty), C.byref(t), None, turn, None) == _lib.OK
    assert call(C.byref(empty), None, None, None, None) == _lib.OK
    assert call(C.byref(empty), None, None, C.byref(_lib.Turn(None, 0.0)), None) == _lib.BAD_ARG


def test_refusals_of_the_whole_body_call():
    keep = []
    call = _lib.lib().bmpc_wb_plan_batch_turn_device
    d, t = _wb_desc(keep), _terrain_desc(keep)
    w = np.zeros(2)
    for terrain in (None, C.byref(t)):
        for bad in BAD_INERTIA:
            assert call(C.byref(d), terrain, None, C.byref(_lib.Turn(w.ctypes.data, bad)), None) == _lib.BAD_ARG, bad
            assert "yaw_inertia" in _lib.last_error(), _lib.last_error()
        assert call(C.byref(d), terrain, None, C.byref(_lib.Turn(None, 0.05)), None) == _lib.BAD_ARG
        assert "bmpc_turn_t.w_des is NULL" in _lib.last_error(), _lib.last_error()
    turn = C.byref(_lib.Turn(w.ctypes.data, 0.05))
    for tn in (turn, None):
        assert call(None, None, None, tn, None) == _lib.BAD_ARG and "null descriptor" in _lib.last_error()
        for kw, word in ((dict(ik_col=5), "sizes"), (dict(x=None), "input"), (dict(w_des=None), "output"), (dict(ik_tasks=None), "output")):
            assert call(C.byref(_wb_desc(keep, **kw)), None, None, tn, None) == _lib.BAD_ARG and word in _lib.last_error(), kw
        bad = _wb_desc(keep)
        bad.foot_frame[2] = 10 ** 6
        assert call(C.byref(bad), None, None, tn, None) == _lib.BAD_ARG and "foot frame" in _lib.last_error()
        for kw, word in ((dict(heights=None), "heights"), (dict(ny=4097), "[2, 4096]"), (dict(x0=float("inf")), "x0")):
            assert call(C.byref(d), C.byref(_terrain_desc(keep, **kw)), None, tn, None) == _lib.BAD_ARG and word in _lib.last_error(), kw
    empty = _wb_desc(keep, B=0)
    assert call(C.byref(empty), None, None, turn, None) == _lib.OK and call(C.byref(empty), C.byref(t), None, None, None) == _lib.OK
    assert call(C.byref(empty), None, None, C.byref(_lib.Turn(None, 0.05)), None) == _lib.BAD_ARG


def test_python_layer_refuses_before_the_gpu():
    with pytest.raises(ValueError, match="yaw_inertia"):
        turn_struct(float("nan"))
    with pytest.raises(ValueError, match="yaw_inertia"):
        turn_struct(0.0)
    assert turn_struct(0.05).w_des is None
