"""GPU tests of the kernels that walk the kinematic tree on robots with ROTATED JOINT PLACEMENTS and OBLIQUE JOINT AXES
(tests/skew_robot.py; references pinned by tests/test_skew_robot_cpu.py).  Solo12 and Go2 have identity placements and axes along
x / y, so on them none of the following runs with a nonzero operand.  Each kernel is compared with the CPU restatements and with
itself on the absorbed twin of the robot (placement rotations folded into the child frames: the identity-placement paths).

Which test executes which branch:
  joint_step, R_identity == 0 (rbd_quad.h)           test_passes_against_the_references[skew_*] (tests/test_ik_passes_gpu.py; quad_pass1 /
                                                     quad_column of the derivative kernels), test_derivative_pass_skew_against_absorbed,
                                                     test_centroidal_state_and_read_back (quad_pass1 on the global-memory model)
  joint_step_r, R_identity == 0 (rbd_quad.h)         the same pass tests (calc_walk / calc_columns -> quad_part_walk), test_whole_solve
  quad_part16, the block under __any (rbd_quad.h)    test_whole_solve[skew] (every joint lane takes it) and test_whole_solve[skew_one]
                                                     (one lane of one quad takes it, its neighbours do not): forward kernels only,
                                                     in the speculative line search and the fused kernel -- the one-problem-per-wave
                                                     schedule walks quad_part, and the test holds them to each other bit for bit
  kin_compute, m.R[i] != I (rbd_device.h)            test_sampler_draw_for_draw
  leg_joint_rotation, R_identity == 0 (id_ctrl.hip)  test_id_controller_rows[skew-*], [skew_one-*] (Newton-Euler recursion and the
                                                     foot offset of the state row)
  rodrigues, a[2] and a[0] a[1] != 0                 every test above on "skew"; alone (identity placements) in
                                                     test_passes_against_the_references[skew_axes_T2_a3.0_problem] and
                                                     test_id_controller_rows[skew_axes-*]
A failure of skew_axes alone points at rodrigues; of skew_one while skew passes at the __any block of quad_part16."""
import ctypes as C

import numpy as np
import pytest

from bunmpc_amd import _lib
from oracle import rbd_np as rb
from tests import ik_passes_np as P, skew_robot as sk
from tests.test_ik_passes_gpu import PassBatch, same_bits
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
NV, NDX, NX = P.NV, P.NDX, P.NX
T7, T7_ABSORBED = "skew_T7_a1.57_node_feas_xreg1", "skew_absorbed_T7_a1.57_node_feas_xreg1"


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / (den if den > 0 else 1.0))


# ------------------------------------------------------------ 1: derivative pass, skew against absorbed ---
def test_derivative_pass_skew_against_absorbed():
    """the workspace of the T = 7 skew case against that of the absorbed case (same seed: identical xs, us, tasks, weights), node by
    node and quantity by quantity, within the tolerance the kernel is held to against the twins on the skew case"""
    cases = {c.name: c for c in P.cases("small")}
    a, b = cases[T7], cases[T7_ABSORBED]
    for k in ("xs", "us", "x0", "dt", "tasks", "state_w", "x_reg", "ctrl_w"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    tol = P.twins_on_case(a)["tol"]
    B, T = a.B, a.T
    got = []
    for case in (a, b):
        pb = PassBatch(case)
        ws = pb.run(0, 1)
        nodes = [[dict(P.unpack_node(ws[i], pb.lay, t, case.dt[i, min(t, T - 1)], T), cost=ws[i, pb.lay["node_cost"] + t],
                       fs=ws[i, pb.lay["fs"] + t * NDX: pb.lay["fs"] + (t + 1) * NDX]) for t in range(T + 1)] for i in range(B)]
        got.append(nodes)
    gap = {q: 0.0 for q in P.DERIV_QUANTITIES}
    for i in range(B):
        for t in range(T + 1):
            for q in P.DERIV_QUANTITIES:
                if q in got[1][i][t]:
                    gap[q] = max(gap[q], P.node_error(got[0][i][t], got[1][i][t], q))
    print("\nSKEW vs ABSORBED %s gap: %s | gap / tol: %s" % (T7, "  ".join("%s %.1e" % kv for kv in gap.items()),
                                                          "  ".join("%s %.2g" % (q, gap[q] / tol[q]) for q in P.DERIV_QUANTITIES)))
    over = {q: (gap[q], tol[q]) for q in P.DERIV_QUANTITIES if not gap[q] <= tol[q]}
    assert not over, over


# ------------------------------------------------------------------------------------- 2: whole solve ---
SCHEDULES = ((0, 0, True, 0), (1 << 30, 0, True, 0), (1 << 30, 1 << 30, True, 1 << 30), (0, 0, False, 1 << 30), (1 << 30, 1 << 30, False, 0), (6, 3, True, 4))


def _solve(case, schedules):
    """bmpc_ik_solve_batch_device on a solve case under each (speculative_below, all_steps, active list, gains_wave_below) with the
    fused kernel off, then once with the whole batch inside the fused kernel: [dict(xs, us, cost, stop, iters, status, trace)]"""
    lib = _lib.lib()
    pb = PassBatch(case)
    pb.desc.maxiter = 100
    B, T, lay = case.B, case.T, pb.lay
    t_off, t_it, t_w = C.c_long(0), C.c_int(0), C.c_int(0)
    lib.bmpc_ik_layout_trace(T, C.byref(t_off), C.byref(t_it), C.byref(t_w))
    assert t_off.value + t_it.value * t_w.value <= lay["total"] and t_w.value >= 3
    stream = pb.torch.cuda.current_stream(pb.device).cuda_stream
    list_ptr = pb.active_list.data_ptr()

    def run():
        pb.ws.zero_()
        _lib.check(lib.bmpc_ik_solve_batch_device(C.byref(pb.desc), C.c_void_p(stream)))
        pb.torch.cuda.synchronize(pb.device)
        ws = pb.ws.cpu().numpy()
        sc = ws[:, lay["scal"]:lay["scal"] + 16]
        return dict(xs=ws[:, lay["xs"]:lay["xs"] + (T + 1) * NX].reshape(B, T + 1, NX).copy(), us=ws[:, lay["us"]:lay["us"] + T * NV].reshape(B, T, NV).copy(),
                    cost=sc[:, P.SCAL["cost"]].copy(), stop=sc[:, P.SCAL["stop"]].copy(), iters=sc[:, P.SCAL["iters"]].astype(np.int64),
                    status=sc[:, P.SCAL["status"]].astype(np.int64),
                    trace=ws[:, t_off.value:t_off.value + t_it.value * t_w.value].reshape(B, t_it.value, t_w.value).copy())

    out = []
    old, old_all, old_gw = lib.bmpc_ik_set_speculative_below(0), lib.bmpc_ik_set_all_steps(0), lib.bmpc_ik_set_gains_wave_below(0)
    old_fd = lib.bmpc_ik_set_fused_direct_max(0)
    try:
        for below, all_steps, use_list, gains in schedules:
            lib.bmpc_ik_set_speculative_below(below)
            lib.bmpc_ik_set_all_steps(all_steps)
            lib.bmpc_ik_set_gains_wave_below(gains)
            pb.desc.active_list = list_ptr if use_list else None
            out.append(run())
        lib.bmpc_ik_set_speculative_below(old)
        lib.bmpc_ik_set_all_steps(old_all)
        lib.bmpc_ik_set_gains_wave_below(old_gw)
        pb.desc.active_list = list_ptr
        lib.bmpc_ik_set_fused_direct_max(16)
        out.append(run())
    finally:
        lib.bmpc_ik_set_speculative_below(old)
        lib.bmpc_ik_set_all_steps(old_all)
        lib.bmpc_ik_set_gains_wave_below(old_gw)
        lib.bmpc_ik_set_fused_direct_max(old_fd)
    return out


def _same_results(a, b, what):
    n = a["iters"]
    assert np.array_equal(n, b["iters"]) and np.array_equal(a["status"], b["status"]), what
    for k in ("xs", "us", "cost", "stop"):
        assert same_bits(a[k], b[k]), (what, k)
    for i in range(len(n)):
        assert np.array_equal(a["trace"][i, :n[i]], b["trace"][i, :n[i]]), (what, i)


def _within_the_numpy_ddp_tolerance(got, i, ref_xs, ref_us, ref_cost):
    """what tests/test_ik_gpu.py::test_ik_matches_numpy_ddp holds the kernel to against the numpy DDP"""
    assert abs(got["cost"][i] - ref_cost) <= 1e-9 * abs(ref_cost), (i, got["cost"][i], ref_cost)
    ex, eu = rel_l2(got["xs"][i].reshape(-1), np.asarray(ref_xs).reshape(-1)), rel_l2(got["us"][i].reshape(-1), np.asarray(ref_us).reshape(-1))
    assert ex < 1e-8 and eu < 1e-6, (i, ex, eu)
    return ex, eu


@pytest.mark.parametrize("name", ["skew", "skew_one"])
def test_whole_solve(name):
    """the solve case of tests/skew_robot.py (on which the numpy DDP takes the same discrete path for both robots:
    tests/test_skew_robot_cpu.py) through bmpc_ik_solve_batch_device.  "skew": under every line-search schedule of
    tests/test_ik_gpu.py::test_line_search_scheduling_does_not_change_results and with the fused kernel on and off, bit for bit; against
    the numpy DDP.  Both robots: against the absorbed twin on the device -- same iterations, status, accepted step lengths and
    regularisation; xs, us, cost within the tolerance the kernel is held to against the numpy DDP."""
    case, twin = sk.solve_case(name), sk.solve_case(name + "_absorbed")
    for k in ("x0", "dt", "tasks", "state_w", "x_reg", "ctrl_w"):
        assert np.array_equal(getattr(case, k), getattr(twin, k)), k
    schedules = SCHEDULES if name == "skew" else SCHEDULES[:2]          # (one problem per wave: quad_part; speculative: quad_part16)
    runs = _solve(case, schedules)
    for j, r in enumerate(runs[1:]):
        _same_results(runs[0], r, "schedule %d" % (j + 1))
    got = runs[0]
    assert np.all(got["status"] == 0) and len(set(got["iters"].tolist())) > 1, (got["status"], got["iters"])
    ab_runs = _solve(twin, SCHEDULES[:1])
    _same_results(ab_runs[0], ab_runs[1], "absorbed, fused")
    ab = ab_runs[0]
    n = got["iters"]
    assert np.array_equal(n, ab["iters"]) and np.array_equal(got["status"], ab["status"])
    worst = [0.0, 0.0]
    for i in range(case.B):
        assert np.array_equal(got["trace"][i, :n[i], 1:3], ab["trace"][i, :n[i], 1:3]), i        # regularisation, accepted step length
        ex, eu = _within_the_numpy_ddp_tolerance(got, i, ab["xs"][i], ab["us"][i], ab["cost"][i])
        worst = [max(worst[0], ex), max(worst[1], eu)]
    print("\nSOLVE %s vs absorbed: iterations %s, xs rel-L2 %.1e, us %.1e" % (name, n.tolist(), worst[0], worst[1]))
    if name == "skew":
        worst = [0.0, 0.0]
        for i, r in enumerate(sk.np_solve(name)):
            assert r["converged"] and n[i] == r["iters"], (i, n[i], r["iters"])
            assert np.array_equal(got["trace"][i, :n[i], 1:3], r["trace"][:, 1:3]), i
            ex, eu = _within_the_numpy_ddp_tolerance(got, i, r["xs"], r["us"], r["cost"])
            worst = [max(worst[0], ex), max(worst[1], eu)]
        print("SOLVE %s vs numpy DDP: xs rel-L2 %.1e, us %.1e" % (name, worst[0], worst[1]))


# ------------------------------------------------------------ 3: centroidal state and the read-back ---
def _centroidal_state(model, x):
    import torch
    from bunmpc_amd.inverse_kinematics_cpp import as_device_model
    dm = as_device_model(model)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    out = torch.zeros((x.shape[0], 9), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().bmpc_ik_centroidal_state_device(dm.h, C.c_void_p(xd.data_ptr()), C.c_void_p(out.data_ptr()), x.shape[0], C.c_void_p(stream)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_centroidal_state_and_read_back():
    """bmpc_ik_centroidal_state_device on 64 random states (joints in +-pi) of "skew" against rbd_np and against the absorbed twin on the
    device, 1e-13 of the largest entry of a state's [com, vcom, L] (the oracles differ by ~1e-15 between the two robots); and the
    com / momentum read-back of a solved InverseKinematics object on the same robot"""
    from bunmpc_amd.inverse_kinematics_cpp import InverseKinematics
    m, a = sk.robot("skew"), sk.robot("skew_absorbed")
    rng = np.random.default_rng(12)
    x = np.zeros((64, NX))
    for i in range(64):
        q = rb.integrate(m, rb.neutral(m), np.concatenate([rng.standard_normal(3), 0.7 * rng.standard_normal(3), np.zeros(12)]))
        q[7:] = rng.uniform(-np.pi, np.pi, 12)
        x[i] = np.concatenate([q, rng.standard_normal(18)])
    got, got_abs = _centroidal_state(m, x), _centroidal_state(a, x)
    worst = [0.0, 0.0]
    for i in range(64):
        k = rb.Kin(m, x[i, :19], x[i, 19:])
        ref = np.concatenate([k.com, k.vcom(), k.centroidal_momentum()[3:]])
        worst = [max(worst[0], rel(got[i], ref)), max(worst[1], rel(got[i], got_abs[i]))]
    print("\nCENTROIDAL STATE skew: vs rbd_np %.1e, vs absorbed on the device %.1e" % tuple(worst))
    assert worst[0] <= 1e-13 and worst[1] <= 1e-13, worst
    # read-back: a regularisation-only problem about a random configuration; com / momentum of its solution
    T = 7
    x_reg = x[0].copy()
    x_reg[19:] = 0.0
    x0 = rb.state_integrate(m, x_reg, 0.2 * rng.standard_normal(36))
    out = []
    for model in (m, a):
        ik = InverseKinematics(model, T)
        ik.add_state_regularization_cost(0, T, 5e-2, "xReg", sk.STATE_WT, x_reg, False)
        ik.add_ctrl_regularization_cost(0, T, 1e-5, "uReg", sk.CTRL_WT, np.zeros(18), False)
        ik.add_state_regularization_cost(0, T, 5e-2, "xReg", sk.STATE_WT, x_reg, True)
        ik.setup_costs(np.full(T, 0.05))
        ik.optimize(x0)
        assert ik.last_stats()["status"] == 0
        out.append((np.array(ik.get_xs()), ik.return_opt_com(), ik.return_opt_mom()))
    xs, com, mom = out[0]
    kin = [rb.Kin(m, s[:19], s[19:]) for s in xs]
    e = (rel(com, [k.com for k in kin]), rel(mom, [k.centroidal_momentum() for k in kin]), rel(com, out[1][1]), rel(mom, out[1][2]))
    print("READ-BACK skew: com %.1e mom %.1e vs rbd_np; com %.1e mom %.1e vs absorbed" % e)
    assert max(e[:2]) <= 1e-13, e
    assert rel(xs, out[1][0]) < 1e-8 and max(e[2:]) < 1e-8, e        # (two solves: as close as the solve test asks of two solves)


# ---------------------------------------------------------------------------------------- 4: sampler ---
def test_sampler_draw_for_draw():
    """tests/test_perturb_gpu.py::test_sampler_matches_the_oracle_draw_for_draw at its B = 70, K = 5 on "skew" (perturb.hip, the only
    consumer of rbd_device.h::kin_compute): the same chosen draw as perturb_np and its state to the 1e-9 of that test; the same chosen
    draw as the absorbed twin on the device and its state to 1e-12"""
    import torch
    from bunmpc_amd import perturbation
    from tests.test_perturb_gpu import FEET, MU, SIGMA
    s = sk.sampler_inputs("skew")
    B, K = s["z"].shape[:2]
    assert (B, K) == (70, 5)
    dev = lambda a: torch.as_tensor(a, device="cuda:0")        # noqa: E731
    got = []
    for name in ("skew", "skew_absorbed"):
        smp = perturbation.PerturbationSampler(sk.robot(name), FEET, MU, SIGMA, draws_per_call=K)
        qn, vn, ch = smp.apply(dev(s["q"]), dev(s["v"]), dev(s["contact"]), dev(s["z"]))
        got.append((qn.cpu().numpy(), vn.cpu().numpy(), ch.cpu().numpy()))
    (qn, vn, ch), (qa, va, cha) = got
    ref = sk.np_sample("skew")
    n_rej, worst = 0, [0.0, 0.0]
    for b in range(B):
        rq, rv, k = ref[b]
        assert ch[b] == k and cha[b] == k, (b, ch[b], cha[b], k)
        n_rej += k != 0
        if k < 0:
            assert np.all(qn[b] == s["q"][b]) and np.all(vn[b] == s["v"][b])
            continue
        rq = rq.copy()
        if np.dot(rq[3:7], qn[b, 3:7]) < 0:
            rq[3:7] = -rq[3:7]                              # same rotation
        e = max(np.abs(qn[b] - rq).max(), np.abs(vn[b] - rv).max())
        assert e < 1e-9, (b, e)
        if np.dot(qa[b, 3:7], qn[b, 3:7]) < 0:
            qa[b, 3:7] = -qa[b, 3:7]
        ea = max(np.abs(qn[b] - qa[b]).max(), np.abs(vn[b] - va[b]).max())
        assert ea < 1e-12, (b, ea)
        worst = [max(worst[0], e), max(worst[1], ea)]
    print("\nSAMPLER skew: vs perturb_np %.1e, vs absorbed on the device %.1e, %d first draws rejected" % (worst[0], worst[1], n_rej))
    assert n_rej > 5                                         # the rejection path was exercised


# --------------------------------------------------------------------------------- 5: ID controller ---
@pytest.mark.parametrize("feet", ["permuted", "mid_leg"])
@pytest.mark.parametrize("name", ["skew", "skew_axes", "skew_one"])
def test_id_controller_rows(name, feet):
    """bmpc_id_batch_device on 65 samples (one past the 64-sample workgroup) against id_np and against the absorbed twin on the device,
    both at the 1e-11 of tests/test_id_gpu.py: motion_to_child and the back-propagation with R[k] carrying the placement, and the
    foot offset of the state row, which rebuilds the chain through leg_joint_rotation"""
    import torch
    from bunmpc_amd import robot_id_controller as ric
    from tests.test_id_gpu import _compare, _oracle, _samples
    eff = sk.FEET_PERMUTED if feet == "permuted" else sk.MID_LEG
    m, a = sk.robot(name), sk.robot(name + "_absorbed")
    s = _samples(m, 65, 41)
    kp, kd = np.linspace(2.0, 4.0, 12), np.linspace(0.05, 0.2, 12)
    t = {k: torch.as_tensor(v, device="cuda:0") for k, v in s.items()}
    got = []
    for model in (m, a):
        ctrl = ric.InverseDynamicsController(model, eff)
        got.append(ric.id_batch_device(ctrl.dev_model, ctrl.foot_frames, kp, kd, t["q_des"], t["v_des"], t["a_des"], t["f"], t["q"], t["v"]))
    _compare(got[0], _oracle(m, eff, s, kp, kd))
    _compare(got[0], {k: v.cpu().numpy() for k, v in got[1].items()})
