"""Contact-conditioned goals on the device (include/bunmpc_goals.h, csrc/cc_goals.hip) against the numpy twin (tests/cc_goal_np.py),
which tests/test_cc_goals_cpu.py holds to recorded outputs of the reference: bit for bit from arrays, and from whole-body states up
to the last bits of the kinematics (1e-12, the bound test_whole_body_plan_on_the_device holds the same kinematics to) with everything
downstream of the device's own intermediates bit for bit again."""
import functools
import os
from dataclasses import replace

import numpy as np
import pytest

from bunmpc_amd import problems, urdf_model
from tests import cc_goal_np as twin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 5
GAITS = {"trot": problems.TROT, "bound": problems.BOUND, "jump": problems.JUMP,           # jump: every foot starts in swing
         "stand": replace(problems.TROT, name="stand", stance_percent=(1.0,) * 4),          # 100 % stance: no switch
         "trot_h1": replace(problems.TROT, name="trot_h1", gait_horizon=1.0)}              # episode_length 7: H_cp = 1, no switch
OUTPUTS = ("goals", "rows", "status", "schedule", "counts", "cnt_plan", "swing_time")


def inputs():
    """five problems: start times on a knot (0, 0.05), off the grid (0.0137), 5e-5 past a phase boundary of the trot's second pair
    (0.05005: in stance by the 1e-4 slack at knot 0 only) and past the episode's end (0.3: start_step >= end_time at 100 steps);
    w_des != 0; problem 1 stands still (v_des = 0: its events coincide in xy)"""
    rng = np.random.default_rng(7)
    t0 = np.array([0.0, 0.05, 0.0137, 0.05005, 0.3])
    com = np.c_[rng.normal(0, 0.02, (B, 2)), 0.22 + rng.normal(0, 0.01, B)]
    feet0 = np.concatenate([problems.SOLO12.feet_xy[None] + rng.normal(0, 0.01, (B, 4, 2)), 0.018 + rng.uniform(0, 0.05, (B, 4, 1))], axis=2)
    hip_off = problems.SOLO12.offsets_xy[None] + rng.normal(0, 0.005, (B, 4, 2))
    v_des = np.c_[rng.uniform(0.05, 0.3, B), rng.uniform(-0.1, 0.1, B), np.zeros(B)]
    v_des[1] = 0.0
    w_des = np.array([0.4, -0.3, 0.0, 0.25, -0.5])
    return dict(t0=t0, com=com, feet0=feet0, hip_off=hip_off, v_des=v_des, w_des=w_des)


@functools.lru_cache(maxsize=None)
def reference(gait, episode_length, goal_horizon, max_rows, max_events, com_rows=False):
    inp = inputs()
    cr = np.random.default_rng(3).normal(0, 0.1, (B, max_rows, 3)) if com_rows else None
    out = twin.cc_goal_batch(GAITS[gait], episode_length, goal_horizon, max_rows, max_events, com_rows=cr, **inp)
    for v in out.values():
        v.setflags(write=False)
    return out, cr


def device(gait, episode_length, goal_horizon, max_rows, max_events, com_rows=None, want_plan=True):
    import torch
    from bunmpc_amd.cc_goal_batch import DeviceCcGoals
    d = DeviceCcGoals(GAITS[gait], episode_length, goal_horizon=goal_horizon, max_rows=max_rows, max_events=max_events,
                      com_rows=com_rows is not None, want_plan=want_plan, **inputs())
    if com_rows is not None:
        d.com_rows.copy_(torch.from_numpy(com_rows))
    d.build()
    torch.cuda.synchronize()
    return d


def assert_equal(d, ref, names=OUTPUTS):
    for k in names:
        got = getattr(d, k).cpu().numpy()
        assert got.shape == ref[k].shape and np.array_equal(got, ref[k]), k


@pytest.mark.parametrize("max_rows", [1, 50])
@pytest.mark.parametrize("goal_horizon", [1, 2, 3])
@pytest.mark.parametrize("gait,episode_length", [("trot", 100), ("bound", 100), ("jump", 100), ("stand", 100), ("trot_h1", 7)])
def test_array_entry_point_equals_the_twin(gait, episode_length, goal_horizon, max_rows):
    ref, _ = reference(gait, episode_length, goal_horizon, max_rows, 40)
    assert ref["cnt_plan"].shape[1] == {"trot": 40, "bound": 47, "jump": 60, "stand": 40, "trot_h1": 1}[gait]
    if gait in ("stand", "trot_h1"):
        assert np.all(ref["status"] == twin.FEW_SWITCHES) and not ref["rows"].any() and not ref["counts"].any()
    else:
        # problems 0-3 have rows (all max_rows of them), problem 4 starts after the episode's end
        assert np.all(ref["status"][:4] == 0) and np.all(ref["rows"][:4] == max_rows) and ref["status"][4] == twin.START_AFTER_END
        assert np.all(ref["counts"].sum(axis=1) >= 8)
        if gait == "jump":
            assert not ref["cnt_plan"][:3, 0, :, 0].any()
        s = ref["schedule"][1]                            # v_des = 0: every event of a foot at one place
        assert np.all(s[:, 1:3, 1:3] == s[:, 0:1, 1:3]) and ref["counts"][1].min() >= 3
    assert_equal(device(gait, episode_length, goal_horizon, max_rows, 40), ref)


def test_slack_at_the_phase_boundary_is_taken_at_knot_0():
    ref, _ = reference("trot", 100, 1, 50, 40)
    assert np.all(ref["cnt_plan"][3, 0, 1:3, 0] == 1) and np.all(ref["cnt_plan"][3, 1, 1:3, 0] == 0)      # 0.05005 in stance, 0.1 not


def test_without_the_plan_and_with_the_callers_com_rows():
    ref, cr = reference("trot", 100, 2, 50, 40, com_rows=True)
    plain, _ = reference("trot", 100, 2, 50, 40)
    assert not np.array_equal(ref["goals"], plain["goals"]) and np.array_equal(ref["rows"], plain["rows"])
    d = device("trot", 100, 2, 50, 40, com_rows=cr, want_plan=False)
    assert d.cnt_plan is None
    assert_equal(d, ref, OUTPUTS[:5])


def test_goal_steps_past_the_schedule_and_reads_of_the_zero_padding():
    """a plan shorter than the episode (gait_horizon 0.07: 21 knots, 1050 steps, at episode_length 1500), so that the rows run up to the
    end of the schedule: two events per foot, N_total = 8.  Goal horizon 3 reads the zero padding; 8 indexes past the schedule once a
    foot has passed its first event, after a number of good rows; 9 does in every row"""
    import torch
    from bunmpc_amd.cc_goal_batch import DeviceCcGoals
    inp = inputs()
    g = replace(problems.TROT, name="short", gait_horizon=0.07)
    for gh in (3, 8, 9):
        ref = twin.cc_goal_batch(g, 1500, gh, 800, 16, **inp)
        start = (inp["t0"] / 0.001).astype(int)
        assert ref["cnt_plan"].shape[1] == 21 and np.all(ref["counts"] == 2)
        if gh == 3:
            assert np.all(ref["status"] == 0) and np.all(ref["rows"] >= 700) and np.all(ref["rows"] < 800)
            t = start[:, None] + np.arange(800)[None]
            pad = (ref["goals"][:, :, 24::3] == -t[:, :, None]) & (np.arange(800)[None, :, None] < ref["rows"][:, None, None])
            assert pad.any(axis=(1, 2)).all()             # a slot of goal step 2 whose time entry is 0 - t: the padding
        else:
            assert np.all(ref["status"] == twin.PAST_SCHEDULE)
            assert np.all((ref["rows"] > 0) & (ref["rows"] < 700)) if gh == 8 else not ref["rows"].any()
        d = DeviceCcGoals(g, 1500, goal_horizon=gh, max_rows=800, max_events=16, want_plan=True, **inp).build()
        torch.cuda.synchronize()
        assert_equal(d, ref)


def test_one_event_too_many_for_max_events():
    ample, _ = reference("trot", 100, 1, 50, 40)
    n = ample["counts"].sum(axis=1)
    cap = int(n.max()) - 1
    ref, _ = reference("trot", 100, 1, 50, cap)
    over = n > cap
    assert over.any() and not over.all() and np.all(ref["status"][over] == twin.EVENTS_OVERFLOW) and not ref["rows"][over].any()
    assert np.array_equal(ref["counts"], ample["counts"]) and np.array_equal(ref["goals"][~over], ample["goals"][~over])
    assert_equal(device("trot", 100, 1, 50, cap), ref)
    tight, _ = reference("trot", 100, 1, 50, 2)           # the smallest capacity the call takes: every foot's list is cut
    assert np.all(tight["status"] == twin.EVENTS_OVERFLOW)
    assert_equal(device("trot", 100, 1, 50, 2), tight)


# ---- from whole-body states -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def solo12():
    from bunmpc_amd.inverse_kinematics_cpp import as_device_model
    model = urdf_model.RobotModel.from_json(open(os.path.join(ROOT, "bunmpc_amd", "robots", "solo12.json")).read())
    return model, as_device_model(model)


def wb_inputs():
    x = twin.wb_states(B)
    return x, np.array([0.0, 0.05, 0.0137, 0.05005, 0.021]), np.c_[np.linspace(0.05, 0.3, B), np.linspace(-0.1, 0.1, B), np.zeros(B)], \
        np.array([0.4, -0.3, 0.0, 0.25, -0.5])


@pytest.mark.parametrize("gait,goal_horizon", [("trot", 2), ("bound", 1), ("jump", 3)])
def test_whole_body_entry_point(solo12, gait, goal_horizon):
    import torch
    from bunmpc_amd.cc_goal_batch import DeviceWbCcGoals
    model, dm = solo12
    x, t0, v_des, w_des = wb_inputs()
    d = DeviceWbCcGoals(dm, GAITS[gait], problems.FEET, problems.HIPS, 100, x, t0, v_des, w_des, goal_horizon=goal_horizon, max_rows=50,
                        max_events=40, want_plan=True).build()
    torch.cuda.synchronize()
    fe = twin.front_end(model, x, problems.FEET, problems.HIPS)
    mid = {k: getattr(d, k).cpu().numpy() for k in ("com", "feet0", "hips", "hip_off")}
    for k, v in mid.items():
        assert np.allclose(v, fe[k], rtol=0, atol=1e-12), (k, np.abs(v - fe[k]).max())
    assert np.abs(fe["hip_off"] - problems.SOLO12.offsets_xy[None]).max(axis=(1, 2)).min() > 0.03      # yawed: the offsets turn with the base
    # downstream of the device's own intermediates: bit for bit
    ref = twin.cc_goal_batch(GAITS[gait], 100, goal_horizon, 50, 40, t0, mid["com"], mid["feet0"], mid["hip_off"], v_des, w_des)
    assert np.all(ref["status"] == 0) and np.all(ref["rows"] == 50)
    assert_equal(d, ref)
    if gait == "trot":
        # end to end with the twin's own kinematics: no rounded value is within 1e-6 of a tie (tests/test_cc_goals_cpu.py), so every
        # rounding falls the same way and every row is compared; what is not rounded carries the kinematics' last bits
        own = twin.cc_goal_batch(GAITS[gait], 100, goal_horizon, 50, 40, t0, fe["com"], fe["feet0"], fe["hip_off"], v_des, w_des)
        for k in ("rows", "status", "counts", "swing_time"):
            assert np.array_equal(getattr(d, k).cpu().numpy(), own[k]), k
        assert np.array_equal(d.cnt_plan.cpu().numpy()[..., 0], own["cnt_plan"][..., 0])
        for k in ("goals", "schedule", "cnt_plan"):
            assert np.allclose(getattr(d, k).cpu().numpy(), own[k], rtol=0, atol=1e-12), k
        assert np.array_equal(d.goals.cpu().numpy()[:, :, 0::3], own["goals"][:, :, 0::3])              # the step counts are exact


def test_plan_label_generator_with_cc_goals(solo12):
    """PlanLabelGenerator(goal_horizon=1), B = 3: cc_goals equal the host path (ContactPlanner + goals.py on the perturbed states the
    generator returns) up to the kinematics' last bits, the data set takes all four groups, and the option off adds no key"""
    import torch
    from bunmpc_amd import contact_planner, dataset, goals
    from bunmpc_amd.datagen import PlanLabelGenerator
    model, _ = solo12
    n = 3
    wb = problems.make_wb_batch(model, n)
    q = torch.as_tensor(wb.x[:, :19], device="cuda:0")
    v = torch.as_tensor(wb.x[:, 19:], device="cuda:0")
    t0 = torch.as_tensor(np.array([0.0, 0.05, 0.1]), device="cuda:0")
    vd = torch.as_tensor(wb.dyn.meta["v_des_body"], device="cuda:0")
    off = PlanLabelGenerator(model).step(q, v, t0, vd, perturb=False)
    assert set(off) == {"states", "actions", "vc_goals", "q0", "v0", "rejected", "solution"}
    gen = PlanLabelGenerator(model, goal_horizon=1)          # episode_length: 3000 unless step() says otherwise
    on = gen.step(q, v, t0, vd, perturb=False, episode_length=200)
    assert set(on) == set(off) | {"cc_goals", "goal_rows", "goal_status"}
    for k in ("states", "actions", "vc_goals"):
        assert torch.equal(on[k], off[k]), k
    R = on["states"].shape[1]
    cc, rows, status = on["cc_goals"].cpu().numpy(), on["goal_rows"].cpu().numpy(), on["goal_status"].cpu().numpy()
    assert cc.shape == (n, R, 12) and np.all(rows == R) and np.all(status == 0)
    planner = contact_planner.ContactPlanner(problems.TROT)
    vdn = wb.dyn.meta["v_des_body"]
    for b in range(n):
        tb = float(t0[b])
        sched, _ = planner.get_contact_schedule(model, None, wb.x[b, :19], wb.x[b, 19:], vdn[b], 0.0, 200, tb)
        est = goals.get_estimated_com(model, wb.x[b, :19], wb.x[b, 19:], vdn[b], 201, 0.001, problems.TROT)
        host = goals.construct_cc_goal(201, 4, sched, est, goal_horizon=1, sim_dt=0.001, start_step=int(tb / 0.001))[:R]
        assert np.array_equal(cc[b, :, 0::3], host[:, 0::3]) and np.allclose(cc[b], host, rtol=0, atol=1e-12), b
    db = dataset.Database(n * R)
    db.append(on["states"].reshape(n * R, 43).cpu().numpy(), on["actions"].reshape(n * R, 12).cpu().numpy(),
              vc_goals=on["vc_goals"].reshape(n * R, 5).cpu().numpy(), cc_goals=cc.reshape(n * R, 12))
    arrs = db.arrays()
    assert set(arrs) == {"states", "vc_goals", "cc_goals", "actions"} and np.array_equal(arrs["cc_goals"], cc.reshape(n * R, 12))
    # com="plan": the CoM rows are those of the planned states
    gen.goal_com, gen._goals = "plan", None               # (the same generator: its solver is built already)
    plan = gen.step(q, v, t0, vd, perturb=False, episode_length=200)
    pc = plan["cc_goals"].cpu().numpy()
    assert np.array_equal(pc[:, :, 0::3], cc[:, :, 0::3]) and not np.array_equal(pc, cc) and np.abs(pc - cc).max() < 0.05
