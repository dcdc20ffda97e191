"""Contact-conditioned goals without a GPU: the host path (bunmpc_amd/goals.py, bunmpc_amd/contact_planner.py) and the numpy twin
(tests/cc_goal_np.py) against recorded outputs of the reference's own functions (tests/golden/cc_goals/cc_goals_ref.npz, written by
tests/golden/make_golden_cc_goals.py), the twin's plan against problems.contact_plan, the second header (include/bunmpc_goals.h)
against its recorded table, and the refusals of the C-ABI."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from bunmpc_amd import _lib, cc_goal_batch, contact_planner, goals, problems, urdf_model
from bunmpc_amd import build as hip_build
from tests import cc_goal_np as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_abi  # noqa: E402

GAITS = {"trot": problems.TROT, "bound": problems.BOUND, "jump": problems.JUMP}


@pytest.fixture(scope="module")
def rec():
    with np.load(os.path.join(ROOT, "tests", "golden", "cc_goals", "cc_goals_ref.npz")) as f:
        return {k: f[k] for k in f.files}


def cases(rec):
    for i in range(int(rec["n_cases"])):
        c = {k[len("c%d_" % i):]: v for k, v in rec.items() if k.startswith("c%d_" % i)}
        p = int(c["plan"])
        c.update({k[len("p%d_" % p):]: v for k, v in rec.items() if k.startswith("p%d_" % p)})
        yield i, c


def test_the_recording_holds_the_cases_it_should(rec):
    """goal horizons 1..3, a start before the first event, between events and after a foot's last one (raises), slots that read
    the zero padding, an index past N_total (raises) -- on trot, bound and jump plans"""
    assert int(rec["n_plans"]) == 6 and int(rec["n_cases"]) == 72
    seen, pads = set(), 0
    for _, c in cases(rec):
        first, gh, start = np.min(c["switches"][:, 1]), int(c["goal_horizon"]), int(c["start_step"])
        seen.add((gh if gh <= 3 else 0, int(c["raised"]), "before" if start < first else "after"))
        if int(c["raised"]) == 0 and gh > 1:
            n = c["schedule"].shape[1]
            counts = [int(np.count_nonzero(c["schedule"][ee, :, 3])) for ee in range(4)]
            for r in range(c["goal"].shape[0]):
                k = [goals.ee_contact_index(start + r, c["schedule"][ee, :, 0]) + gh - 1 for ee in range(4)]
                pads += any(counts[ee] <= k[ee] < n for ee in range(4))
    assert {(g, 0, w) for g in (1, 2, 3) for w in ("before", "after")} <= seen and (1, 1, "after") in seen and (0, 2, "after") in seen
    assert pads > 100


def test_goal_functions_equal_the_recording_bit_for_bit(rec):
    planner = contact_planner.ContactPlanner(problems.TROT)
    for p in range(int(rec["n_plans"])):
        cnt, start, sw, sched = (rec["p%d_%s" % (p, k)] for k in ("cnt_plan", "start", "switches", "schedule"))
        planner.plan = GAITS[("trot", "trot", "bound", "bound", "jump", "jump")[p]]
        got = planner.get_switches(cnt, float(start))
        assert np.array_equal(got, sw) and np.array_equal(twin.switches(cnt, float(start), planner.plan.gait_dt), sw)
        assert np.array_equal(goals.construct_contact_schedule(sw, 4), sched) and np.array_equal(twin.schedule_of(sw)[0], sched)
        for ee in range(4):
            for t, want in zip(rec["p%d_index_t" % p], rec["p%d_index" % p][ee]):
                assert goals.ee_contact_index(t, sched[ee, :, 0]) == want == twin.contact_index(t, sched[ee, :, 0])
    for i, c in cases(rec):
        L, gh, start, est = int(c["goal_length"]), int(c["goal_horizon"]), int(c["start_step"]), c["est_com"]
        n = est.shape[0]
        assert np.array_equal(goals.estimated_com_rows(np.round(c["com3"], 3), c["v_des"], n, 0.001), est), i
        assert np.array_equal(twin.estimated_com(c["com3"], c["v_des"], n), est), i
        args = (L, 4, c["schedule"], est)
        if int(c["raised"]):
            err = {1: ValueError, 2: IndexError}[int(c["raised"])]
            with pytest.raises(err):
                goals.construct_cc_goal(*args, goal_horizon=gh, sim_dt=0.001, start_step=start)
            with pytest.raises(err):
                twin.reference_goal(L, c["switches"], est, gh, start)
        else:
            assert np.array_equal(goals.construct_cc_goal(*args, goal_horizon=gh, sim_dt=0.001, start_step=start), c["goal"]), i
            assert np.array_equal(twin.reference_goal(L, c["switches"], est, gh, start), c["goal"]), i


def test_get_estimated_com_runs_on_the_robot_model():
    model = solo12()
    q = problems.SOLO12_Q0.copy()
    q[0:2] = 0.1234, -0.0456
    est = goals.get_estimated_com(model, q, np.zeros(18), np.array([0.3, -0.1, 0.0]), 7, 0.001, problems.TROT)
    com = twin.front_end(model, np.concatenate([q, np.zeros(18)])[None], problems.FEET, problems.HIPS)["com"][0]
    assert np.array_equal(est, twin.estimated_com(com, np.array([0.3, -0.1, 0.0]), 7)) and np.all(est[:, 2] == 0)


def test_fewer_than_two_switches_raise_in_both():
    planner = contact_planner.ContactPlanner(problems.TROT)
    stand = np.zeros((5, 4, 4))
    stand[:, :, 0] = 1
    one = stand.copy()
    one[0:2, 1, 0] = 0                                   # foot 1 touches down at knot 2: one switch
    for cnt in (stand, one):
        sw = planner.get_switches(cnt, 0.0)
        assert np.ndim(sw) < 2
        with pytest.raises((TypeError, IndexError)):
            goals.construct_contact_schedule(sw, 4)
        with pytest.raises(IndexError):
            twin.reference_goal(100, twin.switches(cnt, 0.0, 0.05), np.zeros((100, 3)), 1, 0)


# ---- the plan: two restatements of one walk ----------------------------------------------------------------------------------------

def solo12():
    return urdf_model.RobotModel.from_json(open(os.path.join(ROOT, "bunmpc_amd", "robots", "solo12.json")).read())


def plan_inputs(B, seed, w=True):
    rng = np.random.default_rng(seed)
    t0 = np.round(rng.uniform(0, 0.5, B), 3)
    com = np.c_[rng.normal(0, 0.02, (B, 2)), 0.22 + rng.normal(0, 0.01, B)]
    feet0 = np.concatenate([problems.SOLO12.feet_xy[None] + rng.normal(0, 0.01, (B, 4, 2)), np.full((B, 4, 1), 0.018)], axis=2)
    hip_off = problems.SOLO12.offsets_xy[None] + rng.normal(0, 0.005, (B, 4, 2))
    v_des = np.c_[rng.uniform(0, 0.3, B), rng.uniform(-0.1, 0.1, B), np.zeros(B)]
    w_des = rng.uniform(-0.5, 0.5, B) if w else np.zeros(B)
    return t0, com, feet0, hip_off, v_des, w_des


@pytest.mark.parametrize("gait", ["trot", "bound", "jump"])
def test_twin_plan_equals_contact_plan(gait):
    """flags, xy and swing_time at every knot (every knot of the planner is gait_dt long: the first-knot dt rule of contact_plan touches
    dt alone); z too, which both set to the foot size"""
    g = GAITS[gait]
    t0, com, feet0, hip_off, v_des, w_des = plan_inputs(12, 3)
    H = twin.plan_knots(g, 100)
    # bound: 20.0 * 100 * 0.001 * 4.0 * 0.3 / 0.05 is 47.99999999999999 in fp64 and int() truncates, as in the reference
    assert H == {"trot": 40, "bound": 47, "jump": 60}[gait] == contact_planner.plan_knots(g, 100) == cc_goal_batch.plan_knots(100, g)
    cnt, swing = twin.raibert_plan(g, H, t0, com, feet0, hip_off, v_des, w_des)
    ref, ref_swing, _ = problems.contact_plan(g, problems.SOLO12, H, t0, np.round(com[:, :2], 3), com[:, 2], np.round(feet0, 3), v_des, w_des,
                                              hip_offsets=hip_off)
    assert np.array_equal(cnt, ref) and np.array_equal(swing, ref_swing)
    assert 0 < cnt[..., 0].mean() < 1


def test_host_planner_equals_the_twin_from_a_state():
    """ContactPlanner (fk_np, GaitPlanner through the C-ABI) and the twin's front end + plan + schedule, on a yawed and pitched base"""
    model = solo12()
    x = twin.wb_states(3)
    fe = twin.front_end(model, x, problems.FEET, problems.HIPS)
    v_des, w_des, t0 = np.array([0.25, -0.05, 0.0]), 0.3, 0.012
    planner = contact_planner.ContactPlanner(problems.TROT)
    for b in range(3):
        sched, cnt = planner.get_contact_schedule(model, None, x[b, :19], x[b, 19:], v_des, w_des, 100, t0)
        com, feet, hips, hip_off = planner.front_end(model, x[b, :19])
        assert np.allclose(hip_off, fe["hip_off"][b], rtol=0, atol=1e-14) and np.allclose(hips, fe["hips"][b], rtol=0, atol=1e-15)
        t = twin.cc_goal_batch(problems.TROT, 100, 1, 101, 64, np.array([t0]), com[None], feet[None], hip_off[None], v_des[None], np.array([w_des]))
        assert np.array_equal(cnt, t["cnt_plan"][0]) and np.array_equal(planner.swing_time, t["swing_time"][0])
        n = sched.shape[1]
        assert n == t["counts"][0].sum() and np.array_equal(sched, t["schedule"][0][:, :n])
        est = goals.get_estimated_com(model, x[b, :19], x[b, 19:], v_des, 101, 0.001, problems.TROT)
        goal = goals.construct_cc_goal(101, 4, sched, est, goal_horizon=1, sim_dt=0.001, start_step=int(t0 / 0.001))
        assert t["status"][0] == 0 and t["rows"][0] == goal.shape[0] > 0 and np.array_equal(goal, t["goals"][0][:goal.shape[0]])


def test_end_to_end_states_are_away_from_rounding_ties():
    """tests/test_cc_goals_gpu.py compares the device's goals from x with the twin's own kinematics, array_equal: that holds while no
    value that is rounded to 3 decimals (CoM xy, feet, hip - CoM) sits within 1e-6 of a tie -- the two kinematics agree to 1e-12"""
    fe = twin.front_end(solo12(), twin.wb_states(5), problems.FEET, problems.HIPS)
    assert twin.distance_to_rounding_tie(fe["pre"]).min() > 1e-6


# ---- the second header ---------------------------------------------------------------------------------------------------------------

def test_goals_header_equals_its_recorded_table():
    """tests/golden/abi_goals.json: tools/record_abi.py's table of include/bunmpc_goals.h; a change of the header is re-recorded and
    reviewed as a diff of the file"""
    with open(os.path.join(ROOT, "tests", "golden", "abi_goals.json")) as f:
        golden = f.read()
    assert record_abi.dump(_lib.HEADERS["bunmpc_goals.h"]) == golden
    table = json.loads(golden)
    assert len(table["functions"]) == 5 and sorted(table["structs"]) == ["bmpc_cc_gait_t", "bmpc_cc_goal_batch_t", "bmpc_cc_goal_wb_batch_t"]


def test_the_first_header_is_untouched_by_the_second():
    first, goals = _lib.HEADERS["bunmpc.h"], _lib.HEADERS["bunmpc_goals.h"]
    assert len(first.functions) == 164 and len(first.structs) == 18
    for cname, pyname in _lib.HEADER_NAMES["bunmpc_goals.h"].items():
        assert getattr(_lib, pyname) is goals.structs[cname] and cname not in first.structs
    assert not set(goals.functions) & set(first.functions)
    assert os.path.join(os.path.dirname(hip_build.INCLUDE), "bunmpc_goals.h") in hip_build.dependencies() and hip_build.INCLUDE in hip_build.dependencies()
    jobs = hip_build.compile_jobs()
    assert jobs[-1] == ("cc_goals", "cc_goals.hip", []) and all(j[1] == "biconvex_admm.hip" for j in jobs[:12])


# ---- refusals through the C-ABI, no GPU ------------------------------------------------------------------------------------------------

def descriptor(**kw):
    d = _lib.CcGoalBatch()
    d.B, d.n_eff, d.episode_length, d.goal_horizon, d.max_rows, d.max_events, d.sim_dt = 4, 4, 100, 1, 50, 32, 0.001
    d.gait = cc_goal_batch.gait_struct(problems.TROT)
    d.n_knots = 40
    for k in ("t0", "com", "feet0", "hip_off", "v_des", "w_des", "goals", "rows", "status", "schedule", "counts"):
        setattr(d, k, 8)                                 # any non-NULL value: a refused call reads no array
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,word", [
    (dict(n_eff=2), "n_eff = 4"), (dict(goal_horizon=0), "goal_horizon"), (dict(max_events=1), "max_events"), (dict(max_rows=0), "max_rows"),
    (dict(B=-1), "B must be"), (dict(B=(1 << 20) + 1), "B must be"), (dict(episode_length=0), "episode_length"), (dict(n_knots=41), "n_knots"),
    (dict(episode_length=7, n_knots=2, sim_dt=0.0), "sim_dt"), (dict(com=None), "com, feet0, hip_off"), (dict(t0=None), "t0, v_des, w_des"),
    (dict(goals=None), "missing output"), (dict(counts=None), "missing output"), (dict(cnt_plan=8), "both or neither"),
    (dict(B=1 << 20, max_rows=1 << 20), "2^40"),
])
def test_refusals_name_the_limit(kw, word):
    rc = _lib.lib().bmpc_cc_goal_batch_device(C.byref(descriptor(**kw)), None)
    assert rc == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()


def test_refusals_of_the_whole_body_call_and_the_pure_functions():
    lib = _lib.lib()
    assert lib.bmpc_cc_goal_batch_device(None, None) == _lib.BAD_ARG and lib.bmpc_cc_goal_wb_batch_device(None, None) == _lib.BAD_ARG
    w = _lib.CcGoalWbBatch()
    w.g = descriptor(com=None, feet0=None, hip_off=None)      # ignored by the whole-body call
    assert lib.bmpc_cc_goal_wb_batch_device(C.byref(w), None) == _lib.BAD_ARG and "null model" in _lib.last_error()
    w.g = descriptor(n_eff=3)
    assert lib.bmpc_cc_goal_wb_batch_device(C.byref(w), None) == _lib.BAD_ARG and "n_eff = 4" in _lib.last_error()
    # B = 0 is no work and no error, without a GPU
    assert lib.bmpc_cc_goal_batch_device(C.byref(descriptor(B=0)), None) == _lib.OK
    assert lib.bmpc_cc_goal_batch_struct_size() == C.sizeof(_lib.CcGoalBatch)
    assert lib.bmpc_cc_goal_wb_batch_struct_size() == C.sizeof(_lib.CcGoalWbBatch)
    for g in GAITS.values():
        for n in (1, 7, 100, 999, 3000):
            assert cc_goal_batch.plan_knots(n, g) == twin.plan_knots(g, n) == contact_planner.plan_knots(g, n)
    assert cc_goal_batch.plan_knots(3000, problems.TROT) == 1200 and cc_goal_batch.plan_knots(3000, problems.BOUND) == 1440
    assert cc_goal_batch.plan_knots(1, problems.TROT) == 0 and cc_goal_batch.plan_knots(999, problems.TROT) == 399      # truncated, not rounded
    assert lib.bmpc_cc_goal_plan_knots(100, 0.001, 2.0, 0.5, 0.0) == -1


def test_dropin_shim():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dropin_contact_planner", os.path.join(ROOT, "bunmpc_amd", "dropin", "contact_planner.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.ContactPlanner is contact_planner.ContactPlanner
