"""Friction cones about per-contact surface normals on the GPU (run with -m gpu): the kernel against its CPU twin
(tests/cone_frame_np.py) in every lanes-per-problem mapping, both foot counts and every form; feasibility of the returned forces in
their tilted cones; world-z normals against the cone kernel, bit for bit; the strides of the normal array; wave-mates at 21 lanes;
DeviceBatch, the handle, the rotation matrices and KinoDynMP; the refusals of the device entry point.

The cases are tests/cone_np.py's (random forces, L_f = 40, mu ~ U[0.05, 0.3]) with normals tilted by up to 25 degrees per problem,
knot and foot: every case takes all three branches and retries in the force loop, and the twin's counts do not move under one ulp of
x_init (tests/test_cone_frame_cpu.py checks both), so no problem is left out.  The bounds are the cone tests' own: counts and step
constants equal, X / F / P below 1e-5, at H = 63 below max(1e-5, K_SPREAD x the twin's own one-ulp spread)."""
import ctypes as C
import os

import numpy as np
import pytest

from bunmpc_amd import _lib, problems
from bunmpc_amd import batch as bb
from bunmpc_amd.biconvex_mpc_cpp import BiconvexMP
from tests import cone_frame_np, cone_np
from tests.test_cone_gpu import CONE, EUCLID, OUT, _drive, _solve as _solve_case
from tests.util import MAPPINGS, assert_matches_twin, knobs, launch_record  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu
CONEF = "biconvex_admm_conef_kernel"
E3 = np.array([0.0, 0.0, 1.0])


def _case(config, H):
    b, mu, warm, iters = cone_np.case(config, H)
    return b, mu, warm, iters, cone_frame_np.normals(b.B, H, b.E)


def _solve(hiplib, knobs, config, H, lanes, form="harness", normals=None):
    """tests/test_cone_gpu.py's _solve about the case's normals, or about `normals` in their place"""
    nrm = _case(config, H)[4]
    b, mu, got = _solve_case(hiplib, knobs, config, H, lanes, form, nrm if normals is None else normals, CONEF)
    return b, mu, nrm, got


def _feasible(F, mu, nrm):
    fn, excess = cone_frame_np.cone_excess(F, mu, nrm)
    print("feasibility: min fn", fn.min(), "worst |ft| - mu fn", excess.max())
    assert fn.min() >= -1e-12 and excess.max() <= 1e-12
    return fn, excess


def _same(a, b):
    for k in OUT:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("H,lanes", MAPPINGS)
@pytest.mark.parametrize("config", cone_np.CONFIGS)
def test_harness_form_matches_the_twin(hiplib, knobs, config, H, lanes):
    b, mu, nrm, got = _solve(hiplib, knobs, config, H, lanes)
    assert_matches_twin(got, cone_frame_np.twin(config, H), cone_frame_np.twin(config, H, perturbed=True) if H == 63 else None, tag="%s %d %d" % (config, H, lanes))


@pytest.mark.parametrize("form", ["raw", "raw_qf"])
@pytest.mark.parametrize("H,lanes", [(15, 16), (20, 21), (20, 32)])
@pytest.mark.parametrize("config", cone_np.CONFIGS)
def test_raw_form_matches_the_twin(hiplib, knobs, config, H, lanes, form):
    b, mu, nrm, got = _solve(hiplib, knobs, config, H, lanes, form)
    assert_matches_twin(got, cone_frame_np.twin(config, H, with_qf=form == "raw_qf"), tag="%s %d %d %s" % (config, H, lanes, form))


@pytest.mark.parametrize("H,lanes", MAPPINGS)
@pytest.mark.parametrize("config", cone_np.CONFIGS)
def test_returned_forces_lie_in_their_cones(hiplib, knobs, config, H, lanes):
    """F is a projection's output: fn >= -1e-12 and |ft| - mu fn <= 1e-12 for every foot, knot and problem"""
    b, mu, nrm, got = _solve(hiplib, knobs, config, H, lanes)
    fn, excess = _feasible(got["F"], mu, nrm)
    if H >= 31:      # ... and some end on the surface
        assert np.any((fn > 0) & (np.abs(excess) < 1e-12))


@pytest.mark.parametrize("H,lanes", [(20, 32), (20, 21)])
@pytest.mark.parametrize("config", cone_np.CONFIGS)
def test_world_z_normals_are_the_cone_kernel(hiplib, knobs, config, H, lanes):
    """normals (0, 0, 1) everywhere: every output equal to the cone kernel's on the same case"""
    b, mu, want = _solve_case(hiplib, knobs, config, H, lanes)
    for shared in (False, True):
        z = np.broadcast_to(E3, ((1 if shared else b.B), H, b.E, 3))
        got = _solve(hiplib, knobs, config, H, lanes, normals=z)[3]
        _same(got, want)
    assert want["stats"][:, 3].sum() > 0


def test_null_normals_launch_the_cone_kernel(hiplib, knobs):
    """a frame struct without normals, or no frame struct: bmpc_biconvex_solve_batch_cone_device itself -- kernel and bits"""
    import torch
    knobs("bmpc_set_three_per_wave", 0)
    b, mu, warm, iters, nrm = _case("solo12_trot", 20)
    dev = bb.DeviceBatch(b, device="cuda:0", num_iters=iters, cone=dict(EUCLID, mu=mu))
    stream = C.c_void_p(torch.cuda.current_stream(dev.device).cuda_stream)
    outs = []
    for frame in ("cone call", None, _lib.ContactFrame()):
        dev.set_warm_start(*warm, L_f=np.full(b.B, cone_np.L_F))
        if frame == "cone call":
            dev.solve()
        else:
            _lib.check(hiplib.bmpc_biconvex_solve_batch_cone_frames_device(C.byref(dev.desc), C.byref(dev.cone), None if frame is None else C.byref(frame), stream))
        outs.append(dev.results())
        assert launch_record(hiplib) == (CONE, 32, 1)
    _same(outs[1], outs[0])
    _same(outs[2], outs[0])
    host = bb.solve_host(b, num_iters=iters, warm=warm, L_f=np.full(b.B, cone_np.L_F), cone=dict(EUCLID, mu=mu, normals=None))
    assert launch_record(hiplib) == (CONE, 32, 1)
    _same(host, outs[0])


@pytest.mark.parametrize("config", cone_np.CONFIGS)
def test_strides_of_the_normals(hiplib, knobs, config):
    """one set of normals shared by the batch (stride 0) against the same values repeated per problem: the same bits"""
    b, nrm = _case(config, 20)[0], _case(config, 20)[4]
    shared = _solve(hiplib, knobs, config, 20, 32, normals=nrm[2:3])[3]
    each = _solve(hiplib, knobs, config, 20, 32, normals=np.repeat(nrm[2:3], b.B, axis=0))[3]
    _same(shared, each)
    assert shared["stats"][:, 3].sum() > 0
    own = _solve(hiplib, knobs, config, 20, 32)[3]
    assert not np.array_equal(own["F"][0], shared["F"][0]) and np.array_equal(own["F"][2], shared["F"][2])


def test_wave_mates_at_21_lanes(hiplib, knobs):
    """problems 0, 1, 2 share a wave in 21-lane segments: with only problem 1's normals changed, 0 and 2 keep every bit and 1 moves"""
    b, mu, nrm, base = _solve(hiplib, knobs, "solo12_trot", 20, 21)
    other = np.array(nrm)
    other[1] = cone_frame_np.normals(b.B, 20, b.E)[4]
    moved = _solve(hiplib, knobs, "solo12_trot", 20, 21, normals=other)[3]
    for k in OUT:
        for i in (0, 2, 3, 4, 5):
            assert np.array_equal(moved[k][i], base[k][i]), (k, i)
    assert not np.array_equal(moved["F"][1], base["F"][1]) and not np.array_equal(moved["X"][1], base["X"][1])


def test_device_batch_carries_the_normals(hiplib, knobs):
    knobs("bmpc_set_three_per_wave", 0)
    for config in cone_np.CONFIGS:
        b, mu, warm, iters, nrm = _case(config, 20)
        for n in (nrm, nrm[3:4]):
            host = bb.solve_host(b, num_iters=iters, warm=warm, L_f=np.full(b.B, cone_np.L_F), cone=dict(EUCLID, mu=mu, normals=n))
            dev = bb.DeviceBatch(b, device="cuda:0", num_iters=iters, cone=dict(EUCLID, mu=mu, normals=n))
            dev.set_warm_start(*warm, L_f=np.full(b.B, cone_np.L_F))
            dev.solve()
            got = dev.results()
            assert launch_record(hiplib) == (CONEF, 32, 1)
            _same(got, host)


def _frame_with_third_row(n):
    """a rotation matrix whose third row is the unit vector n"""
    a = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    return np.stack([a, np.cross(n, a), n])


@pytest.mark.parametrize("config,E", [("solo12_trot", 4), ("biped_walk", 2)])
def test_handle_path(hiplib, config, E):
    """BiconvexMP.set_contact_normals: problem 0 of the B = 1 batch call, bit for bit; the normals survive optimize; the rotation
    matrices' third rows give the same bits; None restores the cone kernel's result"""
    b6, mu, warm, iters, nrm = _case(config, 15)
    raw6 = cone_np.raw_batch(b6)
    b = problems.make_batch(config, 1, H=15)
    raw = {k: v[:1] for k, v in raw6.items()}
    warm1 = tuple(w[:1] for w in warm)
    kw = dict(num_iters=iters, warm=warm1, L_f=np.full(1, cone_np.L_F), raw=raw)
    want = bb.solve_host(b, cone=dict(EUCLID, mu=mu[:1], normals=nrm[:1]), **kw)
    assert launch_record(hiplib) == (CONEF, 16, 1)
    flat = bb.solve_host(b, cone=dict(EUCLID, mu=mu[:1]), **kw)
    assert launch_record(hiplib) == (CONE, 16, 1)
    assert not np.array_equal(flat["F"], want["F"])

    def check(got, ref, tag):
        assert np.array_equal(got["stats"], ref["stats"][0]) and got["L"] == (ref["L_x"][0], ref["L_f"][0]), tag
        for k in "XFP":
            assert np.array_equal(got[k], ref[k][0]), (tag, k)
    mp = BiconvexMP(b.m, 15, E)
    mp.set_rho(b.rho)
    mp.set_cone_projection("euclidean")
    mp.set_friction_coefficients(mu[0])
    mp.set_contact_normals(nrm[0])
    for again in (False, True):      # ... and the normals persist
        got = _drive(mp, b, 0, raw, warm1, iters)
        assert launch_record(hiplib) == (CONEF, 16, 1), again
        check(got, want, again)
    mp.set_contact_normals(None)
    got = _drive(mp, b, 0, raw, warm1, iters)
    assert launch_record(hiplib) == (CONE, 16, 1)
    check(got, flat, "world z")
    # set_rotation_matrix_f on its own: stored and unused
    for t in range(15):
        for n in range(E):
            mp.set_rotation_matrix_f(_frame_with_third_row(nrm[0, t, n]))
    got = _drive(mp, b, 0, raw, warm1, iters)
    assert launch_record(hiplib) == (CONE, 16, 1)
    check(got, flat, "matrices unused")
    mp.use_rotation_matrices_as_contact_frames()
    got = _drive(mp, b, 0, raw, warm1, iters)
    assert launch_record(hiplib) == (CONEF, 16, 1)
    check(got, want, "rotations")


def test_refusals_on_the_device_entry_point(hiplib):
    import torch
    b = problems.make_batch("solo12_trot", 4)
    nrm = np.array(cone_frame_np.normals(4, b.H, 4))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f32 = bb.DeviceBatch(b, device="cuda:0", num_iters=1, precision="f32", cone=dict(EUCLID, normals=nrm))
    with pytest.raises(_lib.BmpcError) as e:
        f32.solve()
    assert e.value.code == _lib.BAD_ARG and "fp64" in str(e.value)
    long = problems.make_batch("solo12_trot", 2, H=64)
    long = bb.DeviceBatch(long, device="cuda:0", num_iters=1, cone=dict(EUCLID, normals=np.array(cone_frame_np.normals(2, 64, 4))))
    with pytest.raises(_lib.BmpcError) as e:
        long.solve()
    assert e.value.code == _lib.BAD_ARG and "64 knots" in str(e.value)
    ok = bb.DeviceBatch(b, device="cuda:0", num_iters=1, cone=dict(EUCLID, normals=nrm))
    cone, frame = ok.cone
    for stride in (-1, 3 * b.H * 4 - 1, (1 << 26) + 1):
        f = _lib.ContactFrame(normals=frame.normals, snormals=stride)
        assert hiplib.bmpc_biconvex_solve_batch_cone_frames_device(C.byref(ok.desc), C.byref(cone), C.byref(f), stream) == _lib.BAD_ARG and "snormals" in _lib.last_error()
    for c in (None, C.byref(_lib.Cone(projection=0))):
        assert hiplib.bmpc_biconvex_solve_batch_cone_frames_device(C.byref(ok.desc), c, C.byref(frame), stream) == _lib.BAD_ARG and "projection = 1" in _lib.last_error()
    ok.desc.n_eff = 3
    assert hiplib.bmpc_biconvex_solve_batch_cone_frames_device(C.byref(ok.desc), C.byref(cone), C.byref(frame), stream) == _lib.BAD_ARG and "n_eff" in _lib.last_error()
    bad = nrm.copy()
    bad[3, 5, 1] *= 1.0 + 1e-6
    with pytest.raises(_lib.BmpcError) as e:
        bb.solve_host(b, num_iters=1, cone=dict(EUCLID, normals=bad))
    assert e.value.code == _lib.BAD_ARG and "unit length" in str(e.value)


def test_scratch_query(hiplib):
    for E in (2, 4):
        s = hiplib.bmpc_biconvex_cone_frame_kernel_scratch_bytes(E)
        print("scratch bytes per lane, n_eff", E, ":", s)
        assert s >= 0


def test_kinodyn_honours_the_handle_or_refuses(hiplib):
    """kd.return_dyn().set_contact_normals(...) is never silently ignored: kd.optimize runs the kernel about the handle's normals, and
    refuses (BMPC_BAD_ARG) a handle the kernels are not built for"""
    from bunmpc_amd import urdf_model
    from bunmpc_amd.biconvex_mpc_cpp import KinoDynMP
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model = urdf_model.RobotModel.from_json(open(os.path.join(root, "bunmpc_amd", "robots", "solo12.json")).read())
    q0 = np.array([0, 0, 0.25, 0, 0, 0, 1] + [0, 0.8, -1.6] * 2 + [0, -0.8, 1.6] * 2, float)
    b = problems.make_batch("solo12_trot_nominal", 1)
    H, T = b.H, 10
    kd = KinoDynMP(model, model.total_mass, 4, H, T)
    kd.set_com_tracking_weight(np.array([0.0]))
    kd.set_mom_tracking_weight(np.array([5e2]))
    mp, ik = kd.return_dyn(), kd.return_ik()
    mp.set_rho(b.rho)
    mu = np.array([0.05, 0.1, 0.15, 0.2])
    nrm = problems.plane_normals(1, H, 4, np.deg2rad(10.0), np.deg2rad(-15.0))[0]

    def load():
        for t in range(H):
            mp.set_contact_plan(b.cnt_plan[0, t], b.dt[0, t])
        mp.create_bound_constraints(b.bounds[0], 15.0, 15.0, 15.0)
        mp.create_cost_X(b.W_X[0], b.W_X_ter[0], b.X_ter[0], b.X_nom[0])
        mp.create_cost_F(b.W_F[0])
        x_reg = np.concatenate([q0, np.zeros(18)])
        ik.add_state_regularization_cost(0, T, 5e-2, "xReg", np.ones(36), x_reg, False)
        ik.add_ctrl_regularization_cost(0, T, 1e-5, "uReg", np.ones(18), np.zeros(18), False)
        ik.add_state_regularization_cost(0, T, 5e-2, "xReg", np.ones(36), x_reg, True)
        ik.add_ctrl_regularization_cost(0, T, 1e-5, "uReg", np.ones(18), np.zeros(18), True)
        ik.setup_costs(b.dt[0, :T])
    load()
    mp.set_cone_projection("euclidean")
    mp.set_friction_coefficients(mu)
    mp.set_contact_normals(nrm)
    kd.optimize(q0, np.zeros(18), 3, 1)
    assert launch_record(hiplib)[0] == CONEF
    F = mp.return_opt_f()
    assert np.any(F != 0)
    _feasible(F, np.broadcast_to(mu, (H, 4)), nrm)
    # normals under the reference's projection: refused, not solved about world z
    load()
    mp.set_cone_projection("reference")
    mp.set_friction_coefficients(0.5)
    with pytest.raises(_lib.BmpcError) as e:
        kd.optimize(q0, np.zeros(18), 3, 1)
    assert e.value.code == _lib.BAD_ARG and "set_cone_projection" in str(e.value)
    # a handle with per-knot blocks: refused (the refused call above left the contact plan in place)
    mp.set_cone_projection("euclidean")
    blk = np.diag(np.tile(b.W_F[0], 1))
    blk[0, 1] = blk[1, 0] = 1e-5
    mp.set_cost_f(blk, np.zeros(mp.nf))
    with pytest.raises(_lib.BmpcError) as e:
        kd.optimize(q0, np.zeros(18), 3, 1)
    assert e.value.code == _lib.BAD_ARG and "diagonal costs only" in str(e.value)
