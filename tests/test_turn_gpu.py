"""Turning commands on the device (include/bunmpc_turn.h; csrc/plan_gen.hip's turn kernels) through every layer: the whole-body and
the centroidal-level plan calls against the numpy builders, BatchedMpc.optimize(w_des=...) against the single-problem harness
(SoloMpcGaitGen.optimize(q, v, t, v_des, w_des)) robot by robot, and PlanLabelGenerator.step(w_des=...).  The batches, the command
vector [0.4, -0.3, 0, 0.25, -0.5, 0] and the seed are those of tests/turn_np.py (tests/test_turn_cpu.py holds the numpy side to the
harness and the seed to its distance from rounding ties)."""
import ctypes as C

import numpy as np
import pytest

from bunmpc_amd import problems
from tests import cc_goal_np as twin
from tests import terrain_np, turn_np
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

B, W_DES = turn_np.B, turn_np.W_DES
WB_OUT = ("x_init", "cnt_plan", "swing_time", "dt", "X_nom", "X_ter", "ik_tasks")
WB_MID = ("com", "feet0", "v_des", "w_des", "hip_off", "amom")
PLAN_OUT = ("cnt_plan", "swing_time", "dt", "X_nom", "X_ter")
CASES = [("trot", False), ("trot", True), ("trot_turn", False), ("trot_turn", True)]


def host(plan, names):
    return {k: getattr(plan, k).cpu().numpy() for k in names if getattr(plan, k) is not None}


def wb_plan(gait, terrain, **kw):
    from bunmpc_amd.inverse_kinematics_cpp import as_device_model
    from bunmpc_amd.plan_batch import DeviceWbPlan
    wb, model = turn_np.batch(gait, False, terrain), turn_np.model()
    g, ik = turn_np.GAITS[gait]
    return DeviceWbPlan(as_device_model(model), g, terrain_np.harness_offsets(model), problems.FEET, ik, wb.x, wb.dyn.meta["t0"],
                        wb.dyn.meta["v_des_body"], wb.dyn.H, wb.ik_T, terrain=turn_np.stairs() if terrain else None, **kw)


# ---- 5. the whole-body plan -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gait,terrain", CASES)
def test_whole_body_plan_with_commands(gait, terrain):
    """DeviceWbPlan(w_des=W_DES) against problems.make_wb_batch(w_des=W_DES) with the tolerances of
    tests/test_plan_gpu.py::test_whole_body_plan_on_the_device (the kinematics differ in their last bits), on flat ground and on the
    stairs, normals included; the rows without a command are the plain call's, bit for bit; turn == NULL is the plain call"""
    from bunmpc_amd import _lib
    import torch
    turn_np.assert_away_from_ties(turn_np.batch(gait).x)
    wb = turn_np.batch(gait, True, terrain)
    Izz = turn_np.yaw_inertia()
    p = wb_plan(gait, terrain, w_des=W_DES, yaw_inertia=Izz).build()
    got = host(p, WB_OUT + WB_MID + ("normals",))
    tol = dict(rtol=0, atol=1e-12)
    for k, ref in (("x_init", wb.dyn.x_init), ("cnt_plan", wb.dyn.cnt_plan), ("X_nom", wb.dyn.X_nom), ("X_ter", wb.dyn.X_ter), ("ik_tasks", wb.ik_tasks)):
        print(gait, terrain, k, np.abs(got[k] - ref).max())
        assert np.allclose(got[k], ref, **tol), k
    assert np.array_equal(got["swing_time"], wb.dyn.swing_time) and np.array_equal(got["dt"], wb.dyn.dt)
    assert np.array_equal(got["w_des"], W_DES)
    turning = W_DES != 0
    Xn = got["X_nom"].reshape(B, -1, 9)
    assert np.all(Xn[turning, :, 8] == (Izz * W_DES[turning])[:, None]) and np.array_equal(got["X_ter"][turning, 8], Izz * W_DES[turning])
    if terrain:
        nrm = got["normals"]
        assert np.abs(nrm - problems.terrain_normals(got["cnt_plan"], turn_np.stairs())).max() <= 4.5e-16
        assert np.abs(np.sum(nrm * nrm, axis=-1) - 1.0).max() <= 1e-9 and got["cnt_plan"][..., 3].max() > 0.018 + 0.02
    # the plain call on the same states: its rows where w == 0, bit for bit, intermediates included
    plain = host(wb_plan(gait, terrain).build(), WB_OUT + WB_MID + ("normals",))
    for k in plain:
        assert np.array_equal(got[k][~turning], plain[k][~turning]), k
        if k in ("cnt_plan", "X_nom", "X_ter", "ik_tasks", "w_des", "amom"):
            assert not np.array_equal(got[k][turning], plain[k][turning]), k      # ... and the commands are not ignored
    # turn == NULL is the plain call, and commands that are all zero give the plain call's plan
    third = wb_plan(gait, terrain)
    for k in WB_OUT + WB_MID:
        getattr(third, k).fill_(float("nan"))
    stream = torch.cuda.current_stream().cuda_stream
    on = third.terrain is not None
    rc = _lib.lib().bmpc_wb_plan_batch_turn_device(C.byref(third.desc), C.byref(third.terrain.desc) if on else None,
                                                       C.c_void_p(third.normals.data_ptr()) if on else None, None, C.c_void_p(stream))
    assert rc == 0
    zeros = host(wb_plan(gait, terrain, w_des=np.zeros(B), yaw_inertia=Izz).build(), WB_OUT + WB_MID + ("normals",))
    null = host(third, WB_OUT + WB_MID + ("normals",))
    for k in plain:
        assert np.array_equal(null[k], plain[k]), k
        assert np.array_equal(zeros[k], plain[k]), k


def test_update_switches_between_the_calls():
    """DeviceWbPlan.update(w_des=...) / update() on one plan object: the commands arrive, and without them the next build is the plain
    call again"""
    Izz = turn_np.yaw_inertia()
    wb = turn_np.batch("trot", False)
    args = (wb.x, wb.dyn.meta["t0"], wb.dyn.meta["v_des_body"])
    plain = host(wb_plan("trot", False).build(), WB_OUT)
    turned = host(wb_plan("trot", False, w_des=W_DES, yaw_inertia=Izz).build(), WB_OUT)
    p = wb_plan("trot", False, yaw_inertia=Izz).build()
    assert all(np.array_equal(v, plain[k]) for k, v in host(p, WB_OUT).items())
    assert all(np.array_equal(v, turned[k]) for k, v in host(p.update(*args, w_des=W_DES).build(), WB_OUT).items())
    assert all(np.array_equal(v, plain[k]) for k, v in host(p.update(*args).build(), WB_OUT).items())
    with pytest.raises(ValueError, match="yaw_inertia"):
        wb_plan("trot", False, w_des=W_DES)
    with pytest.raises(ValueError, match="shape"):
        p.update(*args, w_des=W_DES[:3])


@pytest.mark.parametrize("terrain", [False, True])
def test_a_non_finite_command_spoils_its_own_problem_only(terrain):
    """NaN != 0 and inf != 0: such a command takes the turning branch and gives a non-finite plan -- the numpy builder's, entry for
    entry -- while the other problems of the batch are planned as without it; on the stairs the clamp of the height map takes the
    non-finite locations (no read outside the map), so heights and normals stay finite"""
    W = np.array([np.nan, np.inf, 0.3, 0.0, -np.inf, 0.1])
    ok = np.isfinite(W)
    Izz = turn_np.yaw_inertia()
    names = WB_OUT + ("normals",)
    got = host(wb_plan("trot", terrain, w_des=W, yaw_inertia=Izz).build(), names)
    ref = host(wb_plan("trot", terrain, w_des=np.where(ok, W, 0.0), yaw_inertia=Izz).build(), names)
    for k in got:
        assert np.array_equal(got[k][ok], ref[k][ok]), k
    for k in ("x_init", "dt", "swing_time"):
        assert np.array_equal(got[k][~ok], ref[k][~ok]), k      # what does not depend on the command
    Xn = got["X_nom"].reshape(B, -1, 9)
    assert not np.isfinite(Xn[~ok, :, 8]).any() and not np.isfinite(got["X_ter"][~ok, 8]).any()
    assert not np.isfinite(got["cnt_plan"][~ok]).all(axis=(1, 2, 3)).any()
    g, ik = turn_np.GAITS["trot"]
    with np.errstate(invalid="ignore"):
        wb = problems.make_wb_batch(turn_np.model(), B, seed=turn_np.SEED, gait=g, ik=ik, w_des=W, height_map=turn_np.stairs() if terrain else None)
    for k, r in (("cnt_plan", wb.dyn.cnt_plan), ("X_nom", wb.dyn.X_nom), ("X_ter", wb.dyn.X_ter), ("ik_tasks", wb.ik_tasks)):
        assert np.array_equal(np.isnan(got[k]), np.isnan(r)) and np.array_equal(np.isposinf(got[k]), np.isposinf(r)), k
        assert np.allclose(got[k], r, rtol=0, atol=1e-12, equal_nan=True), k
    if terrain:
        assert np.isfinite(got["normals"]).all() and np.isfinite(got["cnt_plan"][..., 3]).all()


# ---- 6. the centroidal-level plan ---------------------------------------------------------------------------------------------------------------

def centroidal_case(gait, n=B):
    """the construction of tests/test_plan_gpu.py::test_turning_and_off_grid_times (w_des != 0, t0 between knots, amom), every third
    problem without a command"""
    H = gait.horizon
    rng = np.random.default_rng(5)
    t0 = np.round(rng.uniform(0, 0.5, n), 2)
    com = np.c_[rng.normal(0, 0.02, (n, 2)), 0.22 + rng.normal(0, 0.01, n)]
    feet0 = np.concatenate([problems.SOLO12.feet_xy[None] + rng.normal(0, 0.01, (n, 4, 2)), np.full((n, 4, 1), 0.018)], axis=2)
    v_des = np.c_[rng.uniform(0, 0.3, n), rng.uniform(-0.1, 0.1, n), np.zeros(n)]
    w_des = rng.uniform(-0.5, 0.5, n)
    w_des[::3] = 0.0
    x_init = np.c_[com, rng.normal(0, 0.1, (n, 3)), rng.normal(0, 0.02, (n, 3))]
    amom = rng.normal(0, 0.05, (n, 3))
    return dict(gaits=[gait], offsets_xy=problems.SOLO12.offsets_xy, H=H, t0=t0, com=com, feet0=feet0, v_des=v_des, w_des=w_des,
                x_init=x_init, amom=amom)


@pytest.mark.parametrize("gait,terrain", CASES)
def test_centroidal_plan_with_the_yaw_momentum_reference(gait, terrain):
    """DevicePlan(yaw_inertia=...) against contact_plan + centroidal_costs + the override (:602-607): the same bits, as
    test_turning_and_off_grid_times asks of the plain call; turn == NULL is the plain call"""
    from bunmpc_amd import _lib
    from bunmpc_amd.plan_batch import DevicePlan
    import torch
    g = turn_np.GAITS[gait][0]
    inp, Izz = centroidal_case(g), 0.0437
    assert inp["H"] == turn_np.SHAPES[gait][0]
    n, H, w = inp["t0"].shape[0], inp["H"], inp["w_des"]
    hm = terrain_np.terrain("stairs", n) if terrain else None
    cnt, swing, dt = problems.contact_plan(g, problems.SOLO12, H, inp["t0"], np.round(inp["com"][:, :2], 3), inp["com"][:, 2],
                                           np.round(inp["feet0"], 3), inp["v_des"], w, height_map=hm)
    X_nom, X_ter = problems.centroidal_costs(g, H, inp["x_init"], inp["v_des"], dt, inp["amom"])
    plain_ref = dict(cnt_plan=cnt, swing_time=swing, dt=dt, X_nom=X_nom.copy(), X_ter=X_ter.copy())
    turning = w != 0
    X_nom[turning, 8::9] = (Izz * w[turning])[:, None]
    X_ter[turning, 8] = Izz * w[turning]
    ref = dict(plain_ref, X_nom=X_nom, X_ter=X_ter)
    got = host(DevicePlan(terrain=hm, yaw_inertia=Izz, **inp).build(), PLAN_OUT + ("normals",))
    plain = host(DevicePlan(terrain=hm, **inp).build(), PLAN_OUT + ("normals",))
    for k in PLAN_OUT:
        assert np.array_equal(got[k], ref[k]), k
        assert np.array_equal(plain[k], plain_ref[k]), k
    assert not np.array_equal(got["X_nom"], plain["X_nom"]) and 0 < turning.sum() < n
    if terrain:
        assert np.array_equal(got["normals"], plain["normals"]) and np.array_equal(got["normals"], problems.terrain_normals(cnt, hm))
    third = DevicePlan(terrain=hm, **inp)
    for k in PLAN_OUT:
        getattr(third, k).fill_(float("nan"))
    rc = _lib.lib().bmpc_plan_batch_turn_device(C.byref(third.desc), C.byref(third.terrain.desc) if terrain else None,
                                                    C.c_void_p(third.normals.data_ptr()) if terrain else None, None,
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    null = host(third, PLAN_OUT + ("normals",))
    for k in plain:
        assert np.array_equal(null[k], plain[k]), k


# ---- 7. the MPC call ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gait", ["trot", "trot_turn"])
def test_batched_mpc_with_commands_equals_the_harness_call_by_call(gait):
    """BatchedMpc.optimize(w_des=W_DES) against SoloMpcGaitGen.optimize(q, v, t, v_des, w) per robot, with the comparisons and the bound
    of tests/test_harness_gpu.py::test_batched_mpc_equals_the_harness_call_by_call"""
    from bunmpc_amd.cyclic_gen import SoloMpcGaitGen
    from bunmpc_amd.mpc_batch import BatchedMpc
    model, wb = turn_np.model(), turn_np.batch(gait)
    g, ik = turn_np.GAITS[gait]
    t0, vb = wb.dyn.meta["t0"], wb.dyn.meta["v_des_body"]
    mpc = BatchedMpc(model, gait=g, ik=ik, dyn_iters=10)
    assert mpc.yaw_inertia == turn_np.yaw_inertia() and (mpc.H, mpc.T) == turn_np.SHAPES[gait]
    out = mpc.optimize(wb.x, t0, vb, w_des=W_DES)
    rows = out["rows"].cpu().numpy()
    keep = {k: out[k].cpu().numpy() for k in ("xs_int", "us_int", "f_int")}
    gg = SoloMpcGaitGen(model, model, np.concatenate([problems.SOLO12_Q0, np.zeros(18)]), 0.05, problems.SOLO12_Q0)
    for i in range(B):
        gg.update_gait_params(turn_np.params(gait), t0[i])
        q, v = wb.x[i, :19].copy(), wb.x[i, 19:].copy()
        ref = dict(zip(("xs_int", "us_int", "f_int"), gg.optimize(q, v, t0[i], vb[i], W_DES[i], dyn_iters=10)))
        assert rows[i] == ref["xs_int"].shape[0]
        for name, r in ref.items():
            err = rel_l2(keep[name][i, :rows[i]].reshape(-1), r.reshape(-1))
            print(gait, i, name, err)
            assert err < 1e-7, (i, name)
    # the same object without commands: the plain call again, equal to a fresh object that never saw one
    again = mpc.optimize(wb.x, t0, vb)
    fresh = BatchedMpc(model, gait=g, ik=ik, dyn_iters=10).optimize(wb.x, t0, vb)
    import torch
    for k in ("xs_int", "us_int", "f_int", "rows"):
        assert torch.equal(again[k], fresh[k]), k
    assert not np.array_equal(again["xs_int"].cpu().numpy(), keep["xs_int"])


@pytest.mark.parametrize("gait", ["trot", "trot_turn"])
def test_kinodyn_solve_from_device_built_turning_inputs(gait):
    """the KinoDyn solve from the device-built turning inputs against the host-built batch, with the bounds of
    tests/test_plan_gpu.py::test_whole_body_plan_on_the_device"""
    from bunmpc_amd.kinodyn_batch import KinoDynDeviceBatch
    model, wb = turn_np.model(), turn_np.batch(gait)
    p = wb_plan(gait, False, w_des=W_DES, yaw_inertia=turn_np.yaw_inertia()).build()
    a = KinoDynDeviceBatch(wb, model, num_iters=10, plan=p)
    a.solve()
    ra = a.results()
    b = KinoDynDeviceBatch(wb, model, num_iters=10)
    b.solve()
    rb = b.results()
    assert np.array_equal(ra["ik_iters"], rb["ik_iters"]) and np.all(ra["ik_status"] == 0)
    ex, es = rel_l2(ra["X"], rb["X"]), rel_l2(ra["xs"].reshape(B, -1), rb["xs"].reshape(B, -1))
    print(gait, "X", ex.max(), "xs", es.max())
    assert np.all(ex < 1e-9) and np.all(es < 1e-8)


# ---- 8. the label generator ----------------------------------------------------------------------------------------------------------------------

def test_plan_label_generator_with_commands():
    """PlanLabelGenerator.step(w_des=W_DES, goal_horizon=1): vc_goals[:, :, 3] is the command, row for row; cc_goals equal the numpy
    twin's (tests/cc_goal_np.py) run with that w_des from the twin's own kinematics; w_des=None is the generator without the argument"""
    import torch
    from bunmpc_amd import dataset
    from bunmpc_amd.datagen import PlanLabelGenerator
    model, wb = turn_np.model(), turn_np.batch("trot")
    fe = twin.front_end(model, wb.x, problems.FEET, problems.HIPS)
    assert twin.distance_to_rounding_tie(fe["pre"]).min() >= 1e-9
    dev = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda:0")      # noqa: E731
    q, v, t0, vd, w = dev(wb.x[:, :19]), dev(wb.x[:, 19:]), dev(wb.dyn.meta["t0"]), dev(wb.dyn.meta["v_des_body"]), dev(W_DES)
    gen = PlanLabelGenerator(model, goal_horizon=1)
    on = gen.step(q, v, t0, vd, perturb=False, episode_length=600, w_des=w)
    R = on["states"].shape[1]
    vc = on["vc_goals"].cpu().numpy()
    assert R == 50 and np.array_equal(vc[:, :, 3], np.repeat(W_DES[:, None], R, axis=1))
    ref_vc = [dataset.vc_goal_rows(wb.dyn.meta["t0"][b] + 0.001 * np.arange(R), problems.TROT.gait_period, wb.dyn.meta["v_des_body"][b:b + 1], W_DES[b], "trot")
              for b in range(B)]
    assert np.allclose(vc, np.array(ref_vc), rtol=0, atol=1e-12)
    # the MPC call saw the commands: the plan's yaw-momentum reference
    Xn = on["solution"]["plan"].X_nom.cpu().numpy().reshape(B, -1, 9)
    assert np.all(Xn[W_DES != 0, :, 8] == (turn_np.yaw_inertia() * W_DES[W_DES != 0])[:, None])
    cc, rows, status = on["cc_goals"].cpu().numpy(), on["goal_rows"].cpu().numpy(), on["goal_status"].cpu().numpy()
    from bunmpc_amd.cc_goal_batch import default_max_events
    own = twin.cc_goal_batch(problems.TROT, 600, 1, R, default_max_events(problems.TROT, 600), wb.dyn.meta["t0"], fe["com"], fe["feet0"], fe["hip_off"],
                             wb.dyn.meta["v_des_body"], W_DES)
    assert np.all(status == 0) and np.array_equal(status, own["status"]) and np.array_equal(rows, own["rows"]) and np.all(rows == R)
    assert np.array_equal(cc[:, :, 0::3], own["goals"][:, :, 0::3]) and np.allclose(cc, own["goals"], rtol=0, atol=1e-12)
    straight = twin.cc_goal_batch(problems.TROT, 600, 1, R, default_max_events(problems.TROT, 600), wb.dyn.meta["t0"], fe["com"], fe["feet0"], fe["hip_off"],
                                  wb.dyn.meta["v_des_body"], np.zeros(B))
    assert np.abs(own["goals"] - straight["goals"])[W_DES != 0].max() > 1e-4      # the centrifugal term shows in the goals
    # with the nominal plan in the loop (perturb=True) the commands reach it too
    g = torch.Generator(device="cuda:0").manual_seed(3)
    pert = gen.step(q, v, t0, vd, generator=g, episode_length=600, w_des=w)
    assert np.array_equal(gen._nominal.w_des.cpu().numpy(), W_DES) and np.array_equal(pert["vc_goals"][:, :, 3].cpu().numpy(), vc[:, :, 3])
    # w_des=None: the same generator gives what one that never saw a command gives
    off = gen.step(q, v, t0, vd, perturb=False, episode_length=600)
    base = PlanLabelGenerator(model, goal_horizon=1).step(q, v, t0, vd, perturb=False, episode_length=600)
    zero = PlanLabelGenerator(model, goal_horizon=1).step(q, v, t0, vd, perturb=False, episode_length=600, w_des=torch.zeros_like(w))
    assert set(off) == set(base) == set(on)
    for k in ("states", "actions", "vc_goals", "cc_goals", "goal_rows", "goal_status"):
        assert torch.equal(off[k], base[k]), k
        assert torch.equal(zero[k], base[k]), k
    assert torch.all(base["vc_goals"][:, :, 3] == 0) and not torch.equal(on["states"], base["states"])
