"""The Euclidean friction-cone projection with per-foot friction coefficients on the GPU (run with -m gpu): the cone kernel against its
CPU twin (tests/cone_np.py) in every lanes-per-problem mapping, both foot counts and every form; the strides of the coefficient array;
the plain call behind projection 0; feasibility of the returned forces; the Go2 problems the reference's projection cannot solve at
mu = 1; the handle and KinoDynMP paths; the refusals.

The cases (tests/cone_np.py: case) start from random forces and L_f = 40 with mu ~ U[0.05, 0.3] per problem, knot and foot: every case
takes all three branches of the projection and retries in the force loop, and the twin's counts do not move under one ulp of x_init
(tests/test_cone_cpu.py checks both), so no problem is left out.  At H = 63 the horizon amplifies rounding inside the one ADMM
iteration: there the iterates are held to max(1e-5, K_SPREAD x the twin's own one-ulp spread), as in tests/test_band_cost_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

from bunmpc_amd import _lib, problems
from bunmpc_amd import batch as bb
from bunmpc_amd.biconvex_mpc_cpp import BiconvexMP
from tests import cone_np
from tests.util import MAPPINGS, assert_matches_twin, knobs, launch_record  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu
CONE = "biconvex_admm_cone_kernel"
OUT = ("X", "F", "P", "L_x", "L_f", "stats", "dyn_viol")
EUCLID = dict(projection="euclidean")


def _solve(hiplib, knobs, config, H, lanes, form="harness", normals=None, kernel=CONE):
    """the case through `kernel` in the harness form, the raw form or the raw form with a linear force cost; normals: (B or 1, H, E, 3)
    unit vectors for cones about them (tests/test_cone_frame_gpu.py)"""
    knobs("bmpc_set_three_per_wave", 1 if lanes == 21 else 0)
    b, mu, warm, iters = cone_np.case(config, H)
    raw = None if form == "harness" else cone_np.raw_batch(b)
    if form == "raw_qf":
        raw["qf"] = cone_np.linear_force_cost(b)
    cone = dict(EUCLID, mu=mu) if normals is None else dict(EUCLID, mu=mu, normals=normals)
    got = bb.solve_host(b, num_iters=iters, warm=warm, L_f=np.full(b.B, cone_np.L_F), raw=raw, cone=cone)
    assert launch_record(hiplib) == (kernel, lanes, 1)
    return b, mu, got


def _feasible(F, mu):
    F = F.reshape(mu.shape + (3,))
    worst = (np.hypot(F[..., 0], F[..., 1]) - mu * F[..., 2]).max()
    print("feasibility: min fz", F[..., 2].min(), "worst |f_xy| - mu fz", worst)
    assert np.all(F[..., 2] >= 0) and worst <= 1e-12


@pytest.mark.parametrize("H,lanes", MAPPINGS)
@pytest.mark.parametrize("config", cone_np.CONFIGS)
def test_harness_form_matches_the_twin(hiplib, knobs, config, H, lanes):
    b, mu, got = _solve(hiplib, knobs, config, H, lanes, "harness")
    assert_matches_twin(got, cone_np.twin(config, H), cone_np.twin(config, H, perturbed=True) if H == 63 else None, tag="%s %d %d" % (config, H, lanes))


@pytest.mark.parametrize("form", ["raw", "raw_qf"])
@pytest.mark.parametrize("H,lanes", [(15, 16), (20, 21), (20, 32)])
@pytest.mark.parametrize("config", cone_np.CONFIGS)
def test_raw_form_matches_the_twin(hiplib, knobs, config, H, lanes, form):
    b, mu, got = _solve(hiplib, knobs, config, H, lanes, form)
    assert_matches_twin(got, cone_np.twin(config, H, with_qf=form == "raw_qf"), tag="%s %d %d %s" % (config, H, lanes, form))


@pytest.mark.parametrize("H,lanes", MAPPINGS)
@pytest.mark.parametrize("config", cone_np.CONFIGS)
def test_returned_forces_lie_in_their_cones(hiplib, knobs, config, H, lanes):
    """F is a projection's output: fz >= 0 and |f_xy| - mu fz <= 1e-12 for every foot, knot and problem (the twin's worst: 7e-16)"""
    b, mu, got = _solve(hiplib, knobs, config, H, lanes, "harness")
    _feasible(got["F"], mu)
    if H >= 31:      # ... and some end on the surface
        F = got["F"].reshape(mu.shape + (3,))
        assert np.any((F[..., 2] > 0) & (np.abs(np.hypot(F[..., 0], F[..., 1]) - mu * F[..., 2]) < 1e-12))


@pytest.mark.parametrize("config", cone_np.CONFIGS)
def test_strides_of_the_coefficients(hiplib, knobs, config):
    """one set of coefficients shared by the batch (stride 0) against the same values per problem; no array and the scalar 0.2 against an
    array filled with 0.2: the same bits on every output"""
    knobs("bmpc_set_three_per_wave", 0)
    b, mu, warm, iters = cone_np.case(config, 20)
    kw = dict(num_iters=iters, warm=warm, L_f=np.full(b.B, cone_np.L_F))
    pairs = [(dict(cone=dict(EUCLID, mu=mu[2:3])), dict(cone=dict(EUCLID, mu=np.repeat(mu[2:3], b.B, axis=0)))),
             (dict(cone=dict(EUCLID), mu=0.2), dict(cone=dict(EUCLID, mu=np.full(mu.shape, 0.2)))),
             (dict(cone=dict(EUCLID), mu=0.2), dict(cone=dict(EUCLID, mu=np.full((1,) + mu.shape[1:], 0.2)), mu=7.0))]
    for one, other in pairs:
        a = bb.solve_host(b, **kw, **one)
        assert launch_record(hiplib) == (CONE, 32, 1)
        t = bb.solve_host(b, **kw, **other)
        assert launch_record(hiplib) == (CONE, 32, 1)
        for k in OUT:
            assert np.array_equal(a[k], t[k]), k
        assert a["stats"][:, 3].sum() > 0


def test_projection_zero_is_the_plain_call(hiplib):
    """projection 0 without coefficients, or no struct at all: the existing call, kernel and bits -- host and device entry points"""
    import torch
    b = problems.make_batch("solo12_mixed", 9)
    want = bb.solve_host(b, num_iters=3, mu=0.5)
    kernel = launch_record(hiplib)
    assert kernel[0] != CONE
    got = bb.solve_host(b, num_iters=3, mu=0.5, cone=dict(projection="reference"))
    assert launch_record(hiplib) == kernel
    for k in OUT:
        assert np.array_equal(got[k], want[k]), k
    dev = bb.DeviceBatch(b, device="cuda:0", num_iters=3, mu=0.5, cone=dict(projection="reference", mu=None))
    dev.solve()
    got = dev.results()
    assert launch_record(hiplib) == kernel
    stream = C.c_void_p(torch.cuda.current_stream(dev.device).cuda_stream)
    dev.X.zero_()
    _lib.check(hiplib.bmpc_biconvex_solve_batch_cone_device(C.byref(dev.desc), None, stream))
    again = dev.results()
    assert launch_record(hiplib) == kernel
    for k in OUT:
        assert np.array_equal(got[k], want[k]) and np.array_equal(again[k], want[k]), k


def test_go2_at_mu_one(hiplib):
    """go2_bound at the robot's own mu = 1, cold, two ADMM iterations: the plain call overflows to NaN (status 2), the Euclidean
    projection solves all four problems as its twin does"""
    b = problems.make_batch("go2_bound", 4)
    assert b.H == 40
    plain = bb.solve_host(b, num_iters=2, mu=1.0)
    assert launch_record(hiplib)[0] != CONE
    assert np.all(plain["stats"][:, 5] == 2), plain["stats"]
    got = bb.solve_host(b, num_iters=2, mu=1.0, cone=EUCLID)
    assert launch_record(hiplib) == (CONE, 64, 1)
    assert np.all(got["stats"][:, 5] == 0), got["stats"]
    assert_matches_twin(got, [cone_np.restatement(b, i, 2, 1.0) for i in range(4)], tag="go2")
    _feasible(got["F"], np.ones((4, 40, 4)))


def test_device_batch_carries_the_cone(hiplib, knobs):
    knobs("bmpc_set_three_per_wave", 0)
    b, mu, warm, iters = cone_np.case("biped_walk", 20)
    host = bb.solve_host(b, num_iters=iters, warm=warm, L_f=np.full(b.B, cone_np.L_F), cone=dict(EUCLID, mu=mu))
    dev = bb.DeviceBatch(b, device="cuda:0", num_iters=iters, cone=dict(EUCLID, mu=mu))
    dev.set_warm_start(*warm, L_f=np.full(b.B, cone_np.L_F))
    dev.solve()
    got = dev.results()
    assert launch_record(hiplib) == (CONE, 32, 1)
    for k in OUT:
        assert np.array_equal(got[k], host[k]), k


def _drive(mp, b, i, raw, warm, iters):
    for t in range(b.H):
        mp.set_contact_plan(b.cnt_plan[i, t], b.dt[i, t])
    mp.set_bounds_x(raw["lbx"][i], raw["ubx"][i])
    mp.set_cost_x(raw["Qx"][i], raw["qx"][i])
    mp.set_cost_f(raw["Qf"][i], np.zeros(mp.nf))
    mp.set_warm_start_vars(warm[0][i], warm[1][i], warm[2][i])
    mp.set_step_constants(2.25e6, cone_np.L_F)
    mp.optimize(b.x_init[i], iters)
    return dict(X=mp.return_opt_x(), F=mp.return_opt_f(), P=mp.return_opt_p(), stats=mp.last_stats(), L=mp.step_constants())


@pytest.mark.parametrize("config,E", [("solo12_trot", 4), ("biped_walk", 2)])
def test_handle_path(hiplib, config, E):
    """BiconvexMP with set_cone_projection("euclidean") and set_friction_coefficients: problem 0 of the batch solve, bit for bit; both
    settings survive optimize; back to "reference" and the scalar: the plain kernel"""
    b, mu, warm, iters = cone_np.case(config, 15)
    raw = cone_np.raw_batch(b)
    want = bb.solve_host(b, num_iters=iters, warm=warm, L_f=np.full(b.B, cone_np.L_F), raw=raw, cone=dict(EUCLID, mu=mu))
    assert launch_record(hiplib) == (CONE, 16, 1)
    mp = BiconvexMP(b.m, 15, E)
    mp.set_rho(b.rho)
    mp.set_cone_projection("euclidean")
    mp.set_friction_coefficients(mu[0])
    for again in (False, True):
        got = _drive(mp, b, 0, raw, warm, iters)
        assert launch_record(hiplib) == (CONE, 16, 1), again
        assert np.array_equal(got["stats"], want["stats"][0]) and got["L"] == (want["L_x"][0], want["L_f"][0])
        for k in "XFP":
            assert np.array_equal(got[k], want[k][0]), (again, k)
    # one coefficient per foot, and the scalar under the Euclidean projection
    per_foot = bb.solve_host(b, num_iters=iters, warm=warm, L_f=np.full(b.B, cone_np.L_F), raw=raw, cone=dict(EUCLID, mu=np.broadcast_to(mu[0, 0], mu[:1].shape)))
    mp.set_friction_coefficients(mu[0, 0])
    got = _drive(mp, b, 0, raw, warm, iters)
    assert np.array_equal(got["F"], per_foot["F"][0])
    scalar = bb.solve_host(b, num_iters=iters, warm=warm, L_f=np.full(b.B, cone_np.L_F), raw=raw, mu=0.2, cone=EUCLID)
    mp.set_friction_coefficients(0.2)
    got = _drive(mp, b, 0, raw, warm, iters)
    assert launch_record(hiplib)[0] == CONE and np.array_equal(got["F"], scalar["F"][0])
    mp.set_cone_projection("reference")
    _drive(mp, b, 0, raw, warm, iters)
    assert launch_record(hiplib)[0] != CONE


def test_refusals_on_the_device_entry_point(hiplib):
    import torch
    b = problems.make_batch("solo12_trot", 4)
    mu = np.full((4, b.H, 4), 0.2)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dev = bb.DeviceBatch(b, device="cuda:0", num_iters=1, cone=dict(projection="reference", mu=mu))
    with pytest.raises(_lib.BmpcError) as e:
        dev.solve()
    assert e.value.code == _lib.BAD_ARG and "projection = 1" in str(e.value)
    f32 = bb.DeviceBatch(b, device="cuda:0", num_iters=1, precision="f32", cone=EUCLID)
    with pytest.raises(_lib.BmpcError) as e:
        f32.solve()
    assert e.value.code == _lib.BAD_ARG and "fp64" in str(e.value)
    long = bb.DeviceBatch(problems.make_batch("solo12_trot", 2, H=64), device="cuda:0", num_iters=1, cone=EUCLID)
    with pytest.raises(_lib.BmpcError) as e:
        long.solve()
    assert e.value.code == _lib.BAD_ARG and "64 knots" in str(e.value)
    ok = bb.DeviceBatch(b, device="cuda:0", num_iters=1, cone=dict(EUCLID, mu=mu))
    for smu in (-1, b.H * 4 - 1, (1 << 26) + 1):
        c = _lib.Cone(projection=1, mu=ok.t_mu.data_ptr(), smu=smu)
        assert hiplib.bmpc_biconvex_solve_batch_cone_device(C.byref(ok.desc), C.byref(c), stream) == _lib.BAD_ARG and "smu" in _lib.last_error()
    ok.desc.n_eff = 3
    assert hiplib.bmpc_biconvex_solve_batch_cone_device(C.byref(ok.desc), C.byref(ok.cone), stream) == _lib.BAD_ARG and "n_eff" in _lib.last_error()
    with pytest.raises(_lib.BmpcError) as e:
        bb.solve_host(b, num_iters=1, cone=dict(EUCLID, mu=np.where(np.arange(4)[:, None, None] == 3, -0.2, mu)))
    assert e.value.code == _lib.BAD_ARG and "finite and > 0" in str(e.value)


def test_kinodyn_honours_the_handle_or_refuses(hiplib):
    """kd.return_dyn().set_cone_projection(...) is never silently ignored: kd.optimize runs the cone kernel with the handle's
    coefficients, and refuses (BMPC_BAD_ARG) a handle the cone kernels are not built for"""
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
    kd.optimize(q0, np.zeros(18), 3, 1)
    assert launch_record(hiplib)[0] == CONE
    F = mp.return_opt_f()
    assert np.any(F != 0)
    _feasible(F, np.broadcast_to(mu, (H, 4)))
    # a handle with per-knot blocks under the Euclidean projection: refused, not solved with another projection
    load()
    blk = np.diag(np.tile(b.W_F[0], 1))
    blk[0, 1] = blk[1, 0] = 1e-5
    mp.set_cost_f(blk, np.zeros(mp.nf))
    with pytest.raises(_lib.BmpcError) as e:
        kd.optimize(q0, np.zeros(18), 3, 1)
    assert e.value.code == _lib.BAD_ARG and "diagonal costs only" in str(e.value)
