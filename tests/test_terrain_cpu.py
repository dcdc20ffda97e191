"""Terrain height maps without a GPU: bunmpc_amd/terrain.py against analytic planes, the numpy plan builders and the single-problem
harness on a terrain, and every refusal of the terrain entry points straight at the C call (they come before the first HIP call)."""
import ctypes as C
import types

import numpy as np
import pytest

from bunmpc_amd import _lib, problems
from bunmpc_amd.terrain import HeightMap
from tests import terrain_np

EPS = np.finfo(np.float64).eps


# ---- the height map ------------------------------------------------------------------------------------------------------------------

def test_plane_heights_and_normals():
    """A plane whose samples are exact: dyadic cell (2^-5), origin, slopes (3/8, -1/4) and offset, so every node height and every
    difference of neighbours is exact.  Height within 1e-15 of the plane relative to the largest height of the map, and unit normals
    to 1e-15, at random points.  The normal against (-gx, -gy, 1) / |.|:
      * at points on a 1/16-cell grid (nodes, edges, interiors, outside the map excluded) a and b have four bits, every product and
        sum of the contract is exact and only the square root and the divisions round: within 1e-15;
      * at random points gy = (h1 - h0) / cell divides two interpolated heights, each rounded twice (the product a d0 and its sum:
        together at most eps max|Z|), by the cell: within 2 eps max|Z| / cell = 1.7e-14 here (measured 1.5e-15)."""
    gx, gy, z0 = 0.375, -0.25, 0.125
    cell = 2.0 ** -5
    hm = HeightMap.from_function(lambda x, y: z0 + gx * x + gy * y, x0=-1.0, y0=-0.5, cell=cell, nx=96, ny=80)
    want_n = np.array([-gx, -gy, 1.0]) / np.sqrt(gx * gx + gy * gy + 1.0)
    rng = np.random.default_rng(1)
    x, y = rng.uniform(-1.0, -1.0 + 95 * cell, 4000), rng.uniform(-0.5, -0.5 + 79 * cell, 4000)
    h, want = hm.getHeight(x, y), z0 + gx * x + gy * y
    err_h = np.abs(h - want).max() / np.abs(hm.Z).max()
    n = hm.getNormal(x, y)
    err_n, err_unit = np.abs(n - want_n).max(), np.abs(np.sum(n * n, axis=-1) - 1.0).max()
    print("plane, random points: height", err_h, "normal", err_n, "unit", err_unit)
    assert n.shape == (4000, 3)
    assert err_h <= 1e-15 and err_unit <= 1e-15 and err_n <= 2.0 * EPS * np.abs(hm.Z).max() / cell
    xs, ys = -1.0 + rng.integers(0, 95 * 16 + 1, 4000) * cell / 16, -0.5 + rng.integers(0, 79 * 16 + 1, 4000) * cell / 16
    hs, ns = hm.getHeight(xs, ys), hm.getNormal(xs, ys)
    print("plane, 1/16-cell grid: height", np.abs(hs - (z0 + gx * xs + gy * ys)).max(), "normal", np.abs(ns - want_n).max())
    assert np.array_equal(hs, z0 + gx * xs + gy * ys)
    assert np.abs(ns - want_n).max() <= 1e-15 and np.abs(np.sum(ns * ns, axis=-1) - 1.0).max() <= 1e-15


def test_plane_builder_has_the_plane_normals_convention():
    """HeightMap.plane(roll, pitch) is the plane whose normal problems.plane_normals gives.  Its samples are rounded (half an ulp of
    the height each), so a difference of neighbours is off by up to eps max|Z| and the gradient by that over the cell: the bound."""
    roll, pitch = np.deg2rad(10.0), np.deg2rad(-15.0)
    hm = HeightMap.plane(roll, pitch, **terrain_np.GRID)
    want = problems.plane_normals(1, 1, 1, roll, pitch)[0, 0, 0]
    rng = np.random.default_rng(2)
    x, y = rng.uniform(-1.0, 1.5, (2, 500))
    bound = 4.0 * EPS * np.abs(hm.Z).max() / hm.cell
    assert np.abs(hm.getNormal(x, y) - want).max() <= bound
    assert np.abs(hm.getHeight(x, y) + (want[0] * x + want[1] * y) / want[2]).max() <= 8.0 * EPS * np.abs(hm.Z).max()
    assert hm.getHeight(0.0, 0.0) == pytest.approx(0.0, abs=1e-15)


def test_nodes_return_their_heights_exactly():
    """x0 + ix cell is exact for a dyadic grid, so u and v are the node indices.  Every node but the last column / row has a = b = 0
    and returns Z whatever its bits; the last ones have a = 1 (or b = 1): z00 + 1 (z10 - z00), exact for heights on a 2^-20 grid."""
    rng = np.random.default_rng(3)
    Z = rng.standard_normal((9, 12))
    hm = HeightMap(-0.75, 0.5, 0.125, Z)
    X, Y = np.meshgrid(-0.75 + 0.125 * np.arange(12), 0.5 + 0.125 * np.arange(9))
    assert np.array_equal(hm.getHeight(X, Y)[:-1, :-1], Z[:-1, :-1])
    Zd = np.round(Z * 2.0 ** 20) / 2.0 ** 20
    assert np.array_equal(HeightMap(-0.75, 0.5, 0.125, Zd).getHeight(X, Y), Zd)


def test_outside_the_map_is_the_border():
    rng = np.random.default_rng(4)
    hm = HeightMap(0.0, 0.0, 0.1, rng.standard_normal((6, 7)))
    y = rng.uniform(0.0, 0.5, 50)
    x = rng.uniform(0.0, 0.6, 50)
    for far in (1.0, 1e6, 1e300, np.inf):
        assert np.array_equal(hm.getHeight(np.full(50, -far), y), hm.getHeight(np.zeros(50), y))
        assert np.array_equal(hm.getHeight(np.full(50, far), y), hm.getHeight(np.full(50, 6 * 0.1), y))
        assert np.array_equal(hm.getHeight(x, np.full(50, -far)), hm.getHeight(x, np.zeros(50)))
        assert np.array_equal(hm.getHeight(x, np.full(50, far)), hm.getHeight(x, np.full(50, 5 * 0.1)))
        assert np.array_equal(hm.getNormal(np.full(50, far), y), hm.getNormal(np.full(50, 6 * 0.1), y))
    assert hm.getHeight(-5.0, -5.0) == hm.Z[0, 0] and hm.getHeight(5.0, 5.0) == hm.Z[-1, -1] and hm.getHeight(5.0, -5.0) == hm.Z[0, -1]
    assert np.isfinite(hm.getHeight(np.nan, np.nan))      # the clamp drops a NaN: an index inside the map


def test_one_terrain_per_problem():
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((3, 5, 6))
    hm = HeightMap(-0.2, -0.2, 0.1, Z)
    x, y = rng.uniform(-0.3, 0.5, (2, 3, 7))
    h = hm.getHeight(x, y)
    for b in range(3):
        one = HeightMap(-0.2, -0.2, 0.1, Z[b])
        assert np.array_equal(h[b], one.getHeight(x[b], y[b]))
        assert np.array_equal(hm.getNormal(x[b], y[b], problem=np.full(7, b)), one.getNormal(x[b], y[b]))
    with pytest.raises(ValueError):
        hm.getHeight(x[:2], y[:2])
    with pytest.raises(ValueError):
        hm.getHeight(0.0, 0.0, problem=3)


def test_constructor_refusals():
    Z = np.zeros((4, 4))
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError):
            HeightMap(0, 0, 0.1, np.where(np.eye(4) > 0, bad, 0.0))
    for cell in (0.0, -0.1, np.nan, np.inf):
        with pytest.raises(ValueError):
            HeightMap(0, 0, cell, Z)
    for shape in ((1, 4), (4, 1), (4, 4097), (4097, 2), (2, 1, 4)):
        with pytest.raises(ValueError):
            HeightMap(0, 0, 0.1, np.zeros(shape))
    with pytest.raises(ValueError):
        HeightMap(np.inf, 0, 0.1, Z)
    assert HeightMap(0, 0, 0.1, np.zeros((2, 4096))).nx == 4096
    st = HeightMap.stairs(0.05, 0.2, x_start=0.1, x0=0.0, y0=0.0, cell=0.05, nx=16, ny=4)
    assert st.getHeight(0.05, 0.1) == 0.0 and st.getHeight(0.2, 0.1) == 0.05 and st.getHeight(0.4, 0.1) == 0.1


# ---- the numpy plan builders ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", terrain_np.CASES)
def test_no_height_map_is_the_plan_of_today(name):
    inputs, numpy_plan, B = terrain_np.case(name)
    flat = numpy_plan(None)
    if name == "turning":
        cnt, swing, dt = problems.contact_plan(problems.TROT, problems.SOLO12, inputs["H"], inputs["t0"], np.round(inputs["com"][:, :2], 3),
                                               inputs["com"][:, 2], np.round(inputs["feet0"], 3), inputs["v_des"], inputs["w_des"])
    else:
        config = name
        b = problems.make_batch(config, B, H=inputs["H"])
        cnt, swing, dt = b.cnt_plan, b.swing_time, b.dt
        assert b.meta["height_map"] is None
    assert np.array_equal(flat["cnt_plan"], cnt) and np.array_equal(flat["swing_time"], swing) and np.array_equal(flat["dt"], dt)
    # an all-zero map: 0.0 + 0.018 is FOOT_SIZE exactly, and the normals are world z
    zero = numpy_plan(terrain_np.terrain("flat", B))
    for k in flat:
        assert np.array_equal(zero[k], flat[k]), k
    nrm = problems.terrain_normals(zero["cnt_plan"], terrain_np.terrain("flat", B))
    assert nrm.shape == cnt.shape[:3] + (3,) and np.all(nrm == np.array([0.0, 0.0, 1.0]))


@pytest.mark.parametrize("tname", terrain_np.TERRAINS)
@pytest.mark.parametrize("name", terrain_np.CASES)
def test_plan_on_a_terrain(name, tname):
    """knot 0 is the current feet; a continuing stance copies x, y, z; every other knot has z = getHeight(x, y) + FOOT_SIZE; flags, x, y,
    swing flags, dt and the cost references are the flat plan's; the normals are getNormal at every knot"""
    inputs, numpy_plan, B = terrain_np.case(name)
    hm = terrain_np.terrain(tname, B)
    flat, ref = numpy_plan(None), terrain_np.reference(name, tname)
    cnt = ref["cnt_plan"]
    assert np.array_equal(cnt[..., :3], flat["cnt_plan"][..., :3])
    for k in ("swing_time", "dt", "X_nom", "X_ter"):
        assert np.array_equal(ref[k], flat[k]), k
    copy, fresh = terrain_np.transitions(cnt)
    prob = np.broadcast_to(np.arange(B)[:, None, None], copy.shape)
    assert np.array_equal(cnt[:, 0, :, 3], flat["cnt_plan"][:, 0, :, 3])
    assert np.array_equal(cnt[:, 1:][copy[:, 1:]], cnt[:, :-1][copy[:, 1:]])
    assert np.array_equal(cnt[fresh][:, 3], hm.getHeight(cnt[fresh][:, 1], cnt[fresh][:, 2], problem=prob[fresh]) + problems.FOOT_SIZE)
    assert fresh.sum() > 0 and copy.sum() > 0 and not np.array_equal(cnt[..., 3], flat["cnt_plan"][..., 3])
    nrm = ref["normals"]
    assert np.array_equal(nrm, hm.getNormal(cnt[..., 1], cnt[..., 2], problem=prob))
    assert np.abs(np.sum(nrm * nrm, axis=-1) - 1.0).max() <= 1e-15
    if tname == "small":      # the feet stand outside the map: the clamp is taken
        assert np.abs(cnt[..., 1]).max() > 0.1 + 0.05


def test_whole_body_batch_on_a_terrain():
    model = terrain_np.solo12_model()
    hm = terrain_np.terrain("stairs", 4)
    flat, wb = problems.make_wb_batch(model, 4), problems.make_wb_batch(model, 4, height_map=hm)
    assert wb.dyn.meta["height_map"] is hm and flat.dyn.meta["height_map"] is None
    assert np.array_equal(wb.dyn.cnt_plan[..., :3], flat.dyn.cnt_plan[..., :3]) and not np.array_equal(wb.dyn.cnt_plan, flat.dyn.cnt_plan)
    assert np.array_equal(wb.dyn.X_nom, flat.dyn.X_nom) and np.array_equal(wb.x, flat.x)
    # the via tasks keep the absolute step_ht; the stance tasks stand on the terrain
    T = wb.ik_T
    on = wb.dyn.cnt_plan[:, :T, :, 0] == 1
    via = ~on & (wb.dyn.swing_time[:, :T] == 1)
    z = wb.ik_tasks[:, :T, :20].reshape(4, T, 4, 5)[..., 4]
    assert via.sum() > 0 and np.all(z[via] == problems.TROT.step_ht)
    assert np.array_equal(z[on], wb.dyn.cnt_plan[:, :T, :, 3][on])


# ---- the single-problem harness --------------------------------------------------------------------------------------------------------

def _trot_params():
    g, ik = problems.TROT, problems.TROT_IK
    return types.SimpleNamespace(
        gait_period=g.gait_period, stance_percent=list(g.stance_percent), gait_dt=g.gait_dt, phase_offset=list(g.phase_offset),
        step_ht=g.step_ht, nom_ht=g.nom_ht, gait_horizon=g.gait_horizon, W_X=g.W_X, W_X_ter=g.W_X_ter, W_F=g.W_F, rho=g.rho,
        ori_correction=list(g.ori_correction), swing_wt=list(ik["swing_wt"]), cent_wt=list(ik["cent_wt"]), reg_wt=list(ik["reg_wt"]),
        state_wt=ik["state_wt"], ctrl_wt=list(ik["ctrl_wt"]))


class OnlyHeight:
    """the reference's duck type: getHeight of two scalars, nothing else"""

    def __init__(self, hm):
        self.hm, self.calls = hm, 0

    def getHeight(self, x, y):
        assert isinstance(x, float) and isinstance(y, float)
        self.calls += 1
        return float(self.hm.getHeight(x, y))


def _gen(height_map):
    from bunmpc_amd.cyclic_gen import SoloMpcGaitGen
    model = terrain_np.solo12_model()
    x_reg = np.concatenate([problems.SOLO12_Q0, np.zeros(18)])
    return SoloMpcGaitGen(model, model, x_reg, 0.05, problems.SOLO12_Q0, height_map=height_map)


def test_harness_plan_on_a_terrain():
    """SoloMpcGaitGen(height_map=hm).create_cnt_plan is the row of problems.make_wb_batch(height_map=hm), on the Solo12 trot"""
    model = terrain_np.solo12_model()
    hm = terrain_np.terrain("stairs", 3)
    wb = problems.make_wb_batch(model, 3, height_map=hm)
    for height_map in (hm, OnlyHeight(hm)):
        gg = _gen(height_map)
        for i in range(3):
            t0 = wb.dyn.meta["t0"][i]
            gg.update_gait_params(_trot_params(), t0)
            q, v = wb.x[i, :19].copy(), wb.x[i, 19:].copy()
            cnt = gg.create_cnt_plan(q, v, t0, wb.dyn.meta["v_des"][i], 0.0)
            # (the batch rotates the hip offsets in another order of operations: the last bit of x, y, as on flat ground --
            # tests/test_harness_gpu.py compares the two with this bound -- and, through the stairs' slopes, of z)
            assert np.allclose(cnt, wb.dyn.cnt_plan[i], rtol=0, atol=1e-15) and np.array_equal(gg.swing_time, wb.dyn.swing_time[i])
            assert np.array_equal(cnt[..., 0], wb.dyn.cnt_plan[i][..., 0])
            assert np.array_equal(gg.dt_arr, wb.dyn.dt[i])
            copy, fresh = terrain_np.transitions(cnt[None])
            assert np.array_equal(cnt[fresh[0]][:, 3], hm.getHeight(cnt[fresh[0]][:, 1], cnt[fresh[0]][:, 2]) + 0.018)
            assert np.array_equal(cnt[1:][copy[0, 1:]], cnt[:-1][copy[0, 1:]])
            assert np.any(cnt[..., 3] > 0.018 + 0.02)      # some foot is planned onto a step
    assert height_map.calls > 0


def test_harness_refusals():
    hm = terrain_np.terrain("stairs", 3)
    only = OnlyHeight(hm)
    gg = _gen(only)      # an object with only getHeight is accepted ...
    with pytest.raises(ValueError):      # ... but has no normals for the cones
        gg.set_terrain_cones(0.5)
    with pytest.raises(ValueError):
        _gen(None).set_terrain_cones(0.5)
    with pytest.raises(TypeError):
        _gen(object())
    gg = _gen(hm)
    gg.update_gait_params(_trot_params(), 0.0)
    q, v = problems.SOLO12_Q0.copy(), np.zeros(18)
    with pytest.raises(NotImplementedError):
        gg.create_cnt_plan(q, v, 0.0, np.zeros(3), 0.0, noise_std=np.zeros((20, 4, 3)))
    with pytest.raises(NotImplementedError):
        gg.create_cnt_plan(q, v, 0.0, np.zeros(3), 0.0, mcts_x_y_cnt_loc=np.zeros((20, 4, 3)))
    with pytest.raises(NotImplementedError):
        gg.optimize(q, v, 0.0, np.zeros(3), 0.0, v_feet_des=np.zeros(3))
    gg.set_terrain_cones(0.5)      # with getNormal: the handle takes the plan's normals (host-side setters, no GPU)
    cnt = gg.create_cnt_plan(q, v, 0.0, np.array([0.3, 0.0, 0.0]), 0.0)
    assert np.array_equal(gg.contact_normals, hm.getNormal(cnt[:, :, 1], cnt[:, :, 2])) and gg.contact_normals.shape == (gg.horizon, 4, 3)


# ---- the C-ABI without a GPU: every refusal comes before the first HIP call ------------------------------------------------------------

def _plan_desc(keep, B=2, H=4):
    """a plan descriptor whose arrays are host memory: never read, every call below is refused (or has B = 0)"""
    d = _lib.PlanBatch()
    d.B, d.n_col, d.n_gaits = B, H, 1
    buf = np.zeros(4096)
    keep.append(buf)
    for name, _ in _lib.PlanBatch._fields_[4:]:
        if name not in ("gait_id", "amom", "hip_off"):
            setattr(d, name, buf.ctypes.data)
    return d


def _terrain_desc(keep, **kw):
    Z = np.zeros((8, 8))
    keep.append(Z)
    t = _lib.Terrain(nx=8, ny=8, x0=0.0, y0=0.0, cell=0.1, heights=Z.ctypes.data, sheights=0)
    for k, v in kw.items():
        setattr(t, k, v)
    return t


BAD_TERRAINS = [(dict(heights=None), "heights"), (dict(nx=1), "[2, 4096]"), (dict(ny=1), "[2, 4096]"), (dict(nx=4097), "[2, 4096]"),
                (dict(ny=4097), "[2, 4096]"), (dict(cell=0.0), "cell"), (dict(cell=-1.0), "cell"), (dict(cell=float("nan")), "cell"),
                (dict(cell=float("inf")), "cell"), (dict(x0=float("inf")), "x0"), (dict(y0=float("nan")), "y0"), (dict(sheights=-1), "sheights"),
                (dict(sheights=63), "sheights"), (dict(sheights=(1 << 26) + 1), "sheights")]


def test_terrain_struct_and_signatures(hiplib):
    assert hiplib.bmpc_terrain_struct_size() == C.sizeof(_lib.Terrain) == 48
    for name in ("bmpc_plan_batch_terrain_device", "bmpc_wb_plan_batch_terrain_device", "bmpc_kinodyn_solve_batch_cone_device"):
        assert _lib._SIGS[name] == (C.c_int, [C.c_void_p] * 4) and getattr(hiplib, name)
    assert hiplib.bmpc_abi_version() == 2 and hiplib.bmpc_abi_minor_version() == 2


def test_plan_entry_point_refusals(hiplib):
    keep = []
    call = hiplib.bmpc_plan_batch_terrain_device
    d, nrm = _plan_desc(keep), np.zeros(2 * 4 * 4 * 3)
    assert call(C.byref(d), None, nrm.ctypes.data, None) == _lib.BAD_ARG and "null terrain" in _lib.last_error()
    for kw, word in BAD_TERRAINS:
        t = _terrain_desc(keep, **kw)
        assert call(C.byref(d), C.byref(t), nrm.ctypes.data, None) == _lib.BAD_ARG, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    # everything bmpc_plan_batch_device refuses, with its messages
    t = _terrain_desc(keep)
    assert call(None, C.byref(t), None, None) == _lib.BAD_ARG and "null plan descriptor" in _lib.last_error()
    for field, value, word in (("n_col", 0, "n_col < 1"), ("B", -1, "B < 0"), ("gaits", None, "gait"), ("n_gaits", 2, "gait_id"), ("t0", None, "input"),
                               ("cnt_plan", None, "output")):
        bad = _plan_desc(keep)
        setattr(bad, field, value)
        assert call(C.byref(bad), C.byref(t), None, None) == _lib.BAD_ARG and word in _lib.last_error(), field
        assert hiplib.bmpc_plan_batch_device(C.byref(bad), None) == _lib.BAD_ARG and word in _lib.last_error(), field
    # B == 0: nothing to do, with or without normals; the stride of one map exactly and 2^26 are inside the rule
    empty = _plan_desc(keep, B=0)
    for sheights in (0, 64, 1 << 26):
        assert call(C.byref(empty), C.byref(_terrain_desc(keep, sheights=sheights)), None, None) == _lib.OK
    assert call(C.byref(empty), C.byref(_terrain_desc(keep, nx=1)), None, None) == _lib.BAD_ARG      # ... but a bad terrain is still refused


def test_whole_body_plan_entry_point_refusals(hiplib):
    from bunmpc_amd.inverse_kinematics_cpp import as_device_model
    keep = []
    dm = as_device_model(terrain_np.solo12_model())
    d = _lib.WbPlanBatch()
    d.B, d.n_col, d.ik_col, d.model = 2, 4, 2, dm.h
    buf = np.zeros(4096)
    for name in ("gait", "x", "t0", "v_des_body", "com", "feet0", "v_des", "w_des", "hip_off", "amom", "x_init", "cnt_plan", "swing_time", "dt",
                 "X_nom", "X_ter", "ik_tasks"):
        setattr(d, name, buf.ctypes.data)
    for j in range(4):
        d.foot_frame[j] = dm.model.frame_id(problems.FEET[j])
    call = hiplib.bmpc_wb_plan_batch_terrain_device
    assert call(C.byref(d), None, None, None) == _lib.BAD_ARG and "null terrain" in _lib.last_error()
    for kw, word in BAD_TERRAINS:
        assert call(C.byref(d), C.byref(_terrain_desc(keep, **kw)), None, None) == _lib.BAD_ARG and word in _lib.last_error(), kw
    t = _terrain_desc(keep)
    d.ik_col = 5
    assert call(C.byref(d), C.byref(t), None, None) == _lib.BAD_ARG and "sizes" in _lib.last_error()
    d.ik_col, d.B = 2, 0
    assert call(C.byref(d), C.byref(t), None, None) == _lib.OK


def test_kinodyn_cone_entry_point_refusals(hiplib):
    """bmpc_kinodyn_solve_batch_cone_device refuses what the cone entry points refuse, with their messages, before it launches"""
    from bunmpc_amd.inverse_kinematics_cpp import as_device_model
    dm = as_device_model(terrain_np.solo12_model())
    buf = np.zeros(1 << 16)
    d = _lib.KinoDynBatch()
    hiplib.bmpc_batch_defaults(C.byref(d.dyn))
    d.dyn.B, d.dyn.n_col, d.dyn.n_eff, d.dyn.m = 2, 20, 4, 2.5
    for name in ("cnt_plan", "dt", "x_init", "W_X", "W_X_ter", "W_F", "bounds", "X_nom", "X_ter", "X", "F", "P", "L_x", "L_f"):
        setattr(d.dyn, name, buf.ctypes.data)
    d.ik.B, d.ik.n_col, d.ik.model, d.x = 2, 10, dm.h, buf.ctypes.data
    call = hiplib.bmpc_kinodyn_solve_batch_cone_device
    frame = _lib.ContactFrame(normals=buf.ctypes.data, snormals=0)
    assert call(C.byref(d), C.byref(_lib.Cone(projection=0)), C.byref(frame), None) == _lib.BAD_ARG and "projection = 1" in _lib.last_error()
    assert call(C.byref(d), C.byref(_lib.Cone(projection=2)), None, None) == _lib.BAD_ARG and "projection must be" in _lib.last_error()
    cone = _lib.Cone(projection=1)
    assert call(C.byref(d), C.byref(cone), C.byref(_lib.ContactFrame(normals=buf.ctypes.data, snormals=7)), None) == _lib.BAD_ARG and "snormals" in _lib.last_error()
    d.dyn.precision = 1
    assert call(C.byref(d), C.byref(cone), C.byref(frame), None) == _lib.BAD_ARG and "fp64" in _lib.last_error()
    d.dyn.precision, d.dyn.n_col = 0, 64
    assert call(C.byref(d), C.byref(cone), C.byref(frame), None) == _lib.BAD_ARG and "64 knots" in _lib.last_error()
    d.dyn.n_col, d.dyn.n_eff = 20, 2
    assert call(C.byref(d), C.byref(cone), C.byref(frame), None) == _lib.BAD_ARG and "n_eff must be 4" in _lib.last_error()
    d.dyn.n_eff, d.ik.B = 4, 3
    assert call(C.byref(d), C.byref(cone), C.byref(frame), None) == _lib.BAD_ARG and "inconsistent" in _lib.last_error()
    assert call(None, C.byref(cone), None, None) == _lib.BAD_ARG
    d.ik.B = d.dyn.B = 0
    assert call(C.byref(d), C.byref(cone), C.byref(frame), None) == _lib.OK


def test_python_layer_refusals():
    """what needs no GPU of the batch layer: the cone dict's shapes with a scalar mu, BatchedMpc's "terrain" normals"""
    from bunmpc_amd import batch as bb
    from bunmpc_amd.mpc_batch import BatchedMpc
    keep = []
    c = bb._cone_ext(dict(projection="euclidean", mu=0.3), 2, 5, 4, lambda a: keep.append(np.array(a)) or keep[-1].ctypes.data)
    assert c.smu == 0 and keep[0].shape == (1, 5, 4) and np.all(keep[0] == 0.3)
    with pytest.raises(ValueError):
        bb._cone_ext(dict(projection="euclidean", normals=np.zeros((2, 5, 4, 2))), 2, 5, 4, lambda a: 0)
    model = terrain_np.solo12_model()
    with pytest.raises(ValueError):
        BatchedMpc(model, cone=dict(projection="euclidean", normals="terrain"))
    with pytest.raises(ValueError):
        BatchedMpc(model, terrain=terrain_np.terrain("stairs", 3), cone=dict(projection="euclidean", normals="slope"))
