"""Terrain height maps on the GPU (run with -m gpu): the terrain instantiation of the plan kernel against the numpy builders, bit for
bit; the flat map against the plain entry point; the whole-body plan; a slope solved end to end without a host trip of the plan or its
normals; the batched KinoDyn solve with cones; BatchedMpc on stairs against the single-problem harness."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from bunmpc_amd import _lib, problems
from bunmpc_amd import batch as bb
from bunmpc_amd.terrain import HeightMap
from tests import cone_frame_np, terrain_np
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
PLAN = ("cnt_plan", "swing_time", "dt", "X_nom", "X_ter")
E3 = np.array([0.0, 0.0, 1.0])


def _host(p, keys=PLAN + ("normals",)):
    return {k: getattr(p, k).cpu().numpy() for k in keys}


# ---- 1. the device plan against the numpy builder ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("tname", terrain_np.TERRAINS)
@pytest.mark.parametrize("name", terrain_np.CASES)
def test_device_plan_equals_the_numpy_builder(name, tname):
    """cnt_plan, swing_time, dt, X_nom, X_ter: the same bits.  normals: the same bits too -- the device's fp64 square root and
    divisions round as numpy's do (measured on an MI355X over all sixteen cases: largest difference 0), so equality is asserted, not
    the 2 ulp (4.5e-16) a differently rounded sqrt / division would have needed."""
    B = terrain_np.case(name)[2]
    hm = terrain_np.terrain(tname, B)
    ref = terrain_np.reference(name, tname)
    got = _host(terrain_np.device_plan(name, hm))
    for k in PLAN:
        assert np.array_equal(got[k], ref[k]), k
    diff = np.abs(got["normals"] - ref["normals"]).max()
    unit = np.abs(np.sum(got["normals"] ** 2, axis=-1) - 1.0).max()
    print(name, tname, "normals: largest difference", diff, "largest |n.n - 1|", unit, "tilt up to [deg]", np.rad2deg(np.arccos(got["normals"][..., 2].min())))
    assert got["normals"].shape == ref["cnt_plan"].shape[:3] + (3,)
    assert np.array_equal(got["normals"], ref["normals"])
    assert unit <= 1e-9
    assert not np.all(got["normals"] == E3)


# ---- 2. a flat map is no map -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", terrain_np.CASES)
def test_flat_map_equals_no_map(name):
    B = terrain_np.case(name)[2]
    flat = _host(terrain_np.device_plan(name, None), PLAN)
    for hm in (terrain_np.terrain("flat", B), HeightMap(-2.0, -2.0, 0.5, np.zeros((B, 9, 9)))):
        got = _host(terrain_np.device_plan(name, hm))
        for k in PLAN:
            assert np.array_equal(got[k], flat[k]), k
        assert np.all(got["normals"] == E3)
    ref = terrain_np.case(name)[1](None)
    for k in PLAN:
        assert np.array_equal(flat[k], ref[k]), k


def test_normals_are_optional_and_b_zero_is_ok(hiplib):
    """normals == NULL: the plan alone, same bits; B == 0 returns BMPC_OK"""
    import torch
    hm = terrain_np.terrain("stairs", 5)
    p = terrain_np.device_plan("solo12_trot", hm)
    want = _host(p)
    p.cnt_plan.zero_()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(hiplib.bmpc_plan_batch_terrain_device(C.byref(p.desc), C.byref(p.terrain.desc), None, stream))
    assert np.array_equal(p.cnt_plan.cpu().numpy(), want["cnt_plan"])
    p.desc.B = 0
    assert hiplib.bmpc_plan_batch_terrain_device(C.byref(p.desc), C.byref(p.terrain.desc), C.c_void_p(p.normals.data_ptr()), stream) == _lib.OK
    with pytest.raises(ValueError):      # one map per problem needs as many maps as problems
        terrain_np.device_plan("solo12_trot", terrain_np.terrain("bumps", 6))


# ---- 3. the whole-body plan ------------------------------------------------------------------------------------------------------------

def _wb_plan(model, wb, hm, **kw):
    from bunmpc_amd.inverse_kinematics_cpp import as_device_model
    from bunmpc_amd.plan_batch import DeviceWbPlan
    return DeviceWbPlan(as_device_model(model), problems.TROT, terrain_np.harness_offsets(model), problems.FEET, problems.TROT_IK, wb.x,
                        wb.dyn.meta["t0"], wb.dyn.meta["v_des_body"], wb.dyn.H, wb.ik_T, terrain=hm, **kw).build()


def test_whole_body_plan_on_stairs():
    """DeviceWbPlan(terrain=stairs) against problems.make_wb_batch(height_map=stairs), with the tolerances of
    tests/test_plan_gpu.py::test_whole_body_plan_on_the_device (the kinematics differ in their last bits); the via tasks keep step_ht"""
    model = terrain_np.solo12_model()
    B = 4
    hm = terrain_np.terrain("stairs", B)
    wb = problems.make_wb_batch(model, B, height_map=hm)
    p = _wb_plan(model, wb, hm)
    tol = dict(rtol=0, atol=1e-12)
    assert np.allclose(p.x_init.cpu().numpy(), wb.dyn.x_init, **tol)
    cnt = p.cnt_plan.cpu().numpy()
    assert np.allclose(cnt, wb.dyn.cnt_plan, **tol) and np.array_equal(p.swing_time.cpu().numpy(), wb.dyn.swing_time)
    assert np.array_equal(p.dt.cpu().numpy(), wb.dyn.dt)
    assert np.allclose(p.X_nom.cpu().numpy(), wb.dyn.X_nom, **tol) and np.allclose(p.X_ter.cpu().numpy(), wb.dyn.X_ter, **tol)
    tasks = p.ik_tasks.cpu().numpy()
    assert np.allclose(tasks, wb.ik_tasks, **tol)
    T = wb.ik_T
    via = (cnt[:, :T, :, 0] != 1) & (wb.dyn.swing_time[:, :T] == 1)
    assert via.sum() > 0 and np.all(tasks[:, :T, :20].reshape(B, T, 4, 5)[..., 4][via] == problems.TROT.step_ht)
    assert cnt[..., 3].max() > 0.018 + 0.02      # some foot is planned onto a step
    # the normals are the terrain's under the device's own (x, y), to the bound of test 1
    nrm = p.normals.cpu().numpy()
    assert np.abs(nrm - problems.terrain_normals(cnt, hm)).max() <= 4.5e-16 and np.abs(np.sum(nrm * nrm, axis=-1) - 1.0).max() <= 1e-9


# ---- 4. a slope, end to end on the device ------------------------------------------------------------------------------------------------

def _slope_case(B=4, H=20, pitch=np.deg2rad(25.0)):
    """trot problems standing on a plane pitched by 25 degrees: inputs of DevicePlan and the host-built batch of the same plan"""
    hm = HeightMap.plane(0.0, pitch, **terrain_np.GRID)
    b = problems.make_batch("solo12_trot", B, H=H)
    m = b.meta
    feet0 = m["feet0_raw"].copy()
    feet0[:, :, 2] = hm.getHeight(feet0[:, :, 0], feet0[:, :, 1]) + problems.FOOT_SIZE      # feet0 on the plane
    inputs = dict(gaits=m["gait_objs"], offsets_xy=m["robot"].offsets_xy, H=H, t0=m["t0"], com=b.x_init[:, 0:3].copy(), feet0=feet0, v_des=m["v_des"],
                  w_des=m["w_des"], x_init=b.x_init)
    cnt, swing, dt = problems.contact_plan(problems.TROT, m["robot"], H, m["t0"], np.round(b.x_init[:, 0:2], 3), b.x_init[:, 2], np.round(feet0, 3),
                                           m["v_des"], m["w_des"], height_map=hm)
    assert np.array_equal(dt, b.dt)
    return hm, inputs, dataclasses.replace(b, cnt_plan=cnt, swing_time=swing)


def test_slope_end_to_end_on_the_device(hiplib):
    """DevicePlan(terrain) -> DeviceBatch(plan=p, cone=dict(euclidean, mu, normals=p.normals)): plan and normals never leave HBM.
    X / F / P equal solve_host's on the host-built batch with the same normals; the forces lie in the plane's cones to the bound of
    tests/test_cone_frame_gpu.py (fn >= -1e-12, |ft| - mu fn <= 1e-12); the world-z solve of the same plan leaves them by more than
    the 1e-3 of tests/test_cone_frame_cpu.py::test_world_z_cones_slip_on_a_slope"""
    from bunmpc_amd.plan_batch import DevicePlan
    mu = 0.3
    hm, inputs, b = _slope_case()
    p = DevicePlan(terrain=hm, **inputs).build()
    assert np.array_equal(p.cnt_plan.cpu().numpy(), b.cnt_plan)
    nrm = p.normals.cpu().numpy()
    assert np.abs(nrm - problems.plane_normals(b.B, b.H, 4, 0.0, np.deg2rad(25.0))).max() <= 4.0 * np.finfo(float).eps * np.abs(hm.Z).max() / hm.cell
    dev = bb.DeviceBatch(b, device="cuda:0", num_iters=10, plan=p, cone=dict(projection="euclidean", mu=mu, normals=p.normals))
    assert dev.cone[1].normals == p.normals.data_ptr()      # taken as it is: no copy
    dev.solve()
    got = dev.results()
    assert hiplib.bmpc_biconvex_last_kernel_name() == b"biconvex_admm_conef_kernel"
    want = bb.solve_host(b, num_iters=10, cone=dict(projection="euclidean", mu=mu, normals=nrm))
    for k in "XFP":
        assert np.array_equal(got[k], want[k]), k
    fn, ex = cone_frame_np.cone_excess(got["F"], mu, nrm)
    print("terrain cones: min fn", fn.min(), "worst |ft| - mu fn", ex.max(), "largest force", np.abs(got["F"]).max())
    assert np.any(fn > 1e-3) and fn.min() >= -1e-12 and ex.max() <= 1e-12
    flat = bb.DeviceBatch(b, device="cuda:0", num_iters=10, plan=p, cone=dict(projection="euclidean", mu=mu))
    flat.solve()
    fn, ex = cone_frame_np.cone_excess(flat.results()["F"], mu, nrm)
    print("world-z cones on the slope: worst |ft| - mu fn", ex.max())
    assert ex.max() > 1e-3
    for bad in (p.normals.repeat(1, 1, 1, 2)[..., :3], p.normals.float(), p.normals.cpu()):      # not contiguous, not fp64, not on the device
        with pytest.raises(ValueError):
            bb.DeviceBatch(b, device="cuda:0", plan=p, cone=dict(projection="euclidean", mu=mu, normals=bad))


# ---- 5. KinoDyn with cones ---------------------------------------------------------------------------------------------------------------

KD_OUT = ("X", "F", "P", "L_x", "L_f", "stats", "dyn_viol", "xs", "us", "ik_cost", "ik_stop", "ik_iters", "ik_status")


def test_kinodyn_batch_with_cones(hiplib):
    import torch
    from bunmpc_amd.kinodyn_batch import KinoDynDeviceBatch
    model = terrain_np.solo12_model()
    B, mu = 4, 0.6
    hm = terrain_np.terrain("stairs", B)
    wb = problems.make_wb_batch(model, B, height_map=hm)
    p = _wb_plan(model, wb, hm)
    cone = dict(projection="euclidean", mu=mu, normals=p.normals)
    kb = KinoDynDeviceBatch(wb, model, num_iters=10, plan=p, cone=cone)
    kb.solve()
    got = kb.results()
    assert hiplib.bmpc_biconvex_last_kernel_name() == b"biconvex_admm_conef_kernel"
    assert np.all(got["ik_status"] == 0)
    # the centroidal stage is the DeviceBatch cone solve of the same inputs (x_init as the KinoDyn call left it in the plan)
    dev = bb.DeviceBatch(wb.dyn, device="cuda:0", num_iters=10, plan=p, cone=cone)
    dev.solve()
    ref = dev.results()
    for k in "XFP":
        assert np.array_equal(got[k], ref[k]), k
    nrm = p.normals.cpu().numpy()
    fn, ex = cone_frame_np.cone_excess(got["F"], mu, nrm)
    assert np.any(fn > 1e-3) and fn.min() >= -1e-12 and ex.max() <= 1e-12
    # cone=None: the existing call, and the new entry point with a NULL cone, bit for bit
    plain = KinoDynDeviceBatch(wb, model, num_iters=10, plan=p)
    plain.solve()
    a = plain.results()
    assert hiplib.bmpc_biconvex_last_kernel_name() != b"biconvex_admm_conef_kernel"
    stream = C.c_void_p(torch.cuda.current_stream(plain.device).cuda_stream)
    _lib.check(hiplib.bmpc_kinodyn_solve_batch_cone_device(C.byref(plain.desc), None, None, stream))
    c = plain.results()
    for k in KD_OUT:
        assert np.array_equal(a[k], c[k]), k
    assert not np.array_equal(a["F"], got["F"])
    # refusals come through with the cone entry points' messages
    kb.dyn.cone[0].projection = 0
    with pytest.raises(_lib.BmpcError) as e:
        kb.solve()
    assert e.value.code == _lib.BAD_ARG and "projection = 1" in str(e.value)
    kb.dyn.cone[0].projection = 1
    kb.desc.dyn.precision = 1
    with pytest.raises(_lib.BmpcError) as e:
        kb.solve()
    assert e.value.code == _lib.BAD_ARG and "fp64" in str(e.value)


# ---- 6. BatchedMpc on stairs against the single-problem harness ---------------------------------------------------------------------------

@pytest.mark.parametrize("mu", [None, 0.6])
def test_batched_mpc_on_stairs_equals_the_harness(mu):
    """BatchedMpc(terrain=stairs) against SoloMpcGaitGen(height_map=stairs) robot by robot, with the comparisons and tolerances of
    tests/test_harness_gpu.py::test_batched_mpc_equals_the_harness_call_by_call; mu: once more with the terrain's cones on both sides"""
    from bunmpc_amd.cyclic_gen import SoloMpcGaitGen
    from bunmpc_amd.mpc_batch import BatchedMpc
    from tests.test_terrain_cpu import _trot_params
    model = terrain_np.solo12_model()
    B = 3
    hm = terrain_np.terrain("stairs", B)
    wb = problems.make_wb_batch(model, B, height_map=hm)
    t0, vb = wb.dyn.meta["t0"], wb.dyn.meta["v_des_body"]
    cone = None if mu is None else dict(projection="euclidean", mu=mu, normals="terrain")
    out = BatchedMpc(model, dyn_iters=10, terrain=hm, cone=cone).optimize(wb.x, t0, vb)
    x_reg = np.concatenate([problems.SOLO12_Q0, np.zeros(18)])
    gg = SoloMpcGaitGen(model, model, x_reg, 0.05, problems.SOLO12_Q0, height_map=hm)
    if mu is not None:
        gg.set_terrain_cones(mu)
    rows = out["rows"].cpu().numpy()
    plan = out["plan"]
    cnt, nrm = plan.cnt_plan.cpu().numpy(), plan.normals.cpu().numpy()
    for i in range(B):
        gg.update_gait_params(_trot_params(), t0[i])
        q, v = wb.x[i, :19].copy(), wb.x[i, 19:].copy()
        xs_int, us_int, f_int = gg.optimize(q, v, t0[i], vb[i], 0.0, dyn_iters=10)
        assert np.allclose(gg.cnt_plan, cnt[i], rtol=0, atol=1e-12) and gg.cnt_plan[..., 3].max() > 0.018 + 0.02
        if mu is not None:
            assert np.allclose(gg.contact_normals, nrm[i], rtol=0, atol=1e-12)
        assert rows[i] == xs_int.shape[0]
        for name, ref in (("xs_int", xs_int), ("us_int", us_int), ("f_int", f_int)):
            got = out[name][i, :rows[i]].cpu().numpy()
            assert rel_l2(got.reshape(-1), ref.reshape(-1)) < 1e-7, (i, name)
    if mu is not None:      # the forces of both sides lie in the terrain's cones
        fn, ex = cone_frame_np.cone_excess(out["F"].cpu().numpy(), mu, nrm)
        assert fn.min() >= -1e-12 and ex.max() <= 1e-12
