"""CPU side of the rotated-placement / oblique-axis checks (the GPU side is tests/test_skew_robot_gpu.py): the references the kernels
are judged by are pinned here first, on the robots of tests/skew_robot.py --
  1. every oracle gives the same answer on a skewed robot and on its absorbed twin (the placement rotations folded into the child
     frames), to 1e-13 of the largest entry: rbd_np, id_np (rnea, controller torques, policy state rows; permuted feet, mid-leg end
     effectors), bunmpc_amd/fk_np, perturb_np.sample (same chosen draw, same state);
  2. (tests/test_rbd_cpu.py, parametrised over the model: rbd_np against finite differences on the skewed robot)
  3. (tests/test_ik_twin_cpu.py, tests/test_ik_passes_cpu.py: the two IK twins against each other on the skew cases)
  4. teeth: a transposed placement rotation, or a negated a[2], moves the numpy twin's model-dependent derivatives by more than
     1000 x the tolerance the GPU test applies;
  5. the inputs of the GPU solve test: the numpy DDP takes the same discrete path on the skewed robot and on its absorbed twin."""
import copy

import numpy as np
import pytest

from bunmpc_amd import fk_np
from oracle import id_np, rbd_np as rb
from tests import ik_passes_np as P, skew_robot as sk

VARIANTS = ["skew", "skew_axes", "skew_one"]
BOUND = 1e-13


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / (den if den > 0 else 1.0))


def states(model, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q = rb.integrate(model, rb.neutral(model), np.concatenate([rng.standard_normal(3), 0.7 * rng.standard_normal(3), np.zeros(12)]))
        q[7:] = rng.uniform(-np.pi, np.pi, 12)
        out.append((q, rng.standard_normal(18), 3.0 * rng.standard_normal(18)))
    return out


def test_the_skewed_robots_are_what_they_claim():
    solo = sk.solo12()
    m = sk.robot("skew")
    assert list(m.frames) == list(solo.frames) and [f[0] for f in m.frames.values()] == [f[0] for f in solo.frames.values()]
    assert m.joint_names == solo.joint_names and np.array_equal(m.parent, solo.parent) and np.array_equal(m.mass, solo.mass)
    assert P.frame_groups(m) == P.frame_groups(solo)
    for i in range(m.nj):
        assert abs(np.linalg.norm(rb.log3(m.R[i])) - sk.PLACEMENT_ANGLE) < 1e-12 and abs(np.linalg.norm(m.axis[i]) - 1) < 1e-15
        assert 0.05 < np.arccos(np.clip(m.axis[i] @ solo.axis[i], -1, 1)) <= sk.AXIS_ANGLE + 1e-12       # (a turn about an axis not normal to it)
    assert np.all(np.abs(m.axis) > 1e-3) and np.any(m.axis < 0)
    ax = sk.robot("skew_axes")
    assert np.array_equal(ax.R, solo.R) and np.all(np.abs(ax.axis) > 1e-3) and np.array_equal(ax.com, solo.com)
    one = sk.robot("skew_one")
    assert [i for i in range(12) if not np.array_equal(one.R[i], np.eye(3))] == [4] and np.array_equal(one.axis, solo.axis)
    for name in VARIANTS:
        assert np.array_equal(sk.robot(name + "_absorbed").R, np.tile(np.eye(3), (12, 1, 1)))       # exactly: the kernels test R == I bit for bit
    # a dropped placement rotation is not a rounding matter: the same foot at the same joint angles, centimetres apart
    q = states(m, 1, 0)[0][0]
    assert np.abs(rb.Kin(m, q).frame_placement("FL_FOOT")[1] - rb.Kin(solo, q).frame_placement("FL_FOOT")[1]).max() > 0.05


@pytest.mark.parametrize("name", VARIANTS)
def test_oracles_agree_on_a_skewed_robot_and_its_absorbed_twin(name):
    m, a = sk.robot(name), sk.robot(name + "_absorbed")
    worst = {}

    def note(key, x, y):
        worst[key] = max(worst.get(key, 0.0), rel(x, y))

    sts = states(m, 20, 5)
    frames = ("FL_FOOT", "HR_FOOT", "FR_HFE", "HL_UPPER_LEG", "base_link")
    for q, v, acc in sts:
        k1, k2 = rb.Kin(m, q, v), rb.Kin(a, q, v)
        for f in frames:
            note("frame position", k1.frame_placement(f)[1], k2.frame_placement(f)[1])
            note("frame Jacobian", k1.frame_jacobian_lin(f), k2.frame_jacobian_lin(f))
        note("com", k1.com, k2.com)
        note("com Jacobian", k1.jacobian_com(), k2.jacobian_com())
        note("centroidal map", k1.centroidal_map(), k2.centroidal_map())
        note("dh_dq", k1.dh_dq(), k2.dh_dq())
        note("centroidal momentum", k1.centroidal_momentum(), k2.centroidal_momentum())
        note("rnea", id_np.rnea(m, q, v, acc), id_np.rnea(a, q, v, acc))
    # the controller and the policy state row: the feet in another order, end effectors on any body of a leg; the quaternion of the
    # desired state not of unit length, as between the knots of a plan
    rng = np.random.default_rng(6)
    for feet in (sk.FEET_PERMUTED, sk.MID_LEG):
        c1, c2 = id_np.InverseDynamicsController(m, feet), id_np.InverseDynamicsController(a, feet)
        for c in (c1, c2):
            c.set_gains(np.linspace(2.0, 4.0, 12), np.linspace(0.05, 0.2, 12))
        for q, v, acc in sts[:8]:
            qd = q.copy()
            qd[3:7] *= 0.995
            qm, vm, f = rb.integrate(m, q, 0.05 * rng.standard_normal(18)), rng.standard_normal(18), 8.0 * rng.standard_normal(12)
            t1, t2 = c1.id_joint_torques(qm, vm, qd, v, acc, f), c2.id_joint_torques(qm, vm, qd, v, acc, f)
            note("controller torques", t1[0], t2[0])
            assert np.array_equal(t1[1], t2[1])
            note("policy state", id_np.policy_state(m, qm, vm, feet), id_np.policy_state(a, qm, vm, feet))
    Q, V = np.array([s[0] for s in sts]), np.array([s[1] for s in sts])
    f1, f2 = fk_np.kinematics(m, Q, V), fk_np.kinematics(a, Q, V)
    for key in ("com", "vcom", "L"):
        note("fk_np " + key, f1[key], f2[key])
    note("fk_np frames", fk_np.frame_positions(m, f1, frames), fk_np.frame_positions(a, f2, frames))
    kin = [rb.Kin(m, s[0], s[1]) for s in sts]                          # (and fk_np against rbd_np: they share no code)
    note("fk_np vs rbd_np", f1["L"], np.array([k.centroidal_momentum()[3:] for k in kin]))
    note("fk_np vs rbd_np", fk_np.frame_positions(m, f1, frames), np.array([[k.frame_placement(f)[1] for f in frames] for k in kin]))
    # the sampler: same chosen draw, same state
    B = 70 if name == "skew" else 12
    r1, r2 = sk.np_sample(name, B), sk.np_sample(name + "_absorbed", B)
    assert [r[2] for r in r1] == [r[2] for r in r2]
    for (q1, v1, k1), (q2, v2, _) in zip(r1, r2):
        if k1 >= 0:
            note("sampled q", q1, q2)
            note("sampled v", v1, v2)
    print("skew vs absorbed %-10s %s" % (name, "  ".join("%s %.1e" % kv for kv in worst.items())))
    over = {k: e for k, e in worst.items() if not e <= BOUND}
    assert not over, over


def test_sampler_inputs_exercise_the_rejection_path():
    """tests/test_skew_robot_gpu.py keeps the `n_rej > 5` condition of test_sampler_matches_the_oracle_draw_for_draw: the oracle alone
    must meet it on these inputs (and most problems must end with an accepted draw, so that states are compared at all)"""
    ch = np.array([r[2] for r in sk.np_sample("skew")])
    assert (ch != 0).sum() > 5 and (ch >= 0).sum() > 35, ch.tolist()


# ------------------------------------------------------------------------------- 4: teeth ---
T7 = "skew_T7_a1.57_node_feas_xreg1"
MODEL_DEPENDENT = ("cost", "Lx", "Lxx")


@pytest.mark.parametrize("kind", ["R_transposed", "a2_negated"])
def test_a_wrong_model_lies_far_outside_the_tolerance(kind):
    """The numpy twin on the T = 7 skew case with every R[i] transposed / with a[2] of every axis negated, against itself on the true
    model, in units of the tolerance tests/test_ik_passes_gpu.py applies (tw["tol"]).  The robot enters a node only through its cost
    terms -- cost, L_x, L_xx: each of them must move by more than 1e3 tolerances.  xnext, F_x, F_u (the Euler step on the state
    manifold), L_u, L_uu (the control cost) and the gaps (state differences) do not contain the robot at all: they must not move by a
    bit, and no wrong model can show in them."""
    case = {c.name: c for c in P.cases("small")}[T7]
    tw = P.twins_on_case(case)
    wrong = copy.copy(case)
    wrong.model = sk.wrong_models(case.model)[kind]
    moved = {q: 0.0 for q in P.DERIV_QUANTITIES}
    probs = {}
    for b, t in case.np_nodes():
        if b not in probs:
            probs[b] = wrong.np_problem(b)
        ref = tw["np"][(b, t)]
        mut = P.np_twin_node(probs[b], wrong, b, t)
        prev = case.x0[b] if t == 0 else tw["np"][(b, t - 1)]["xnext"]
        mut["fs"] = rb.state_diff(wrong.model, case.xs[b, t], prev)
        for q in P.DERIV_QUANTITIES:
            if q in ref:
                moved[q] = max(moved[q], P.node_error(mut, ref, q) / tw["tol"][q])
    print("wrong model %-13s moved / tolerance: %s" % (kind, "  ".join("%s %.1e" % kv for kv in moved.items())))
    for q in P.DERIV_QUANTITIES:
        if q in MODEL_DEPENDENT:
            assert moved[q] > 1e3, (q, moved[q])
        else:
            assert moved[q] == 0.0, (q, moved[q])


# ---------------------------------------------------------------- 5: inputs of the solve test ---
@pytest.mark.parametrize("name", ["skew", "skew_one"])
def test_numpy_ddp_takes_the_same_path_on_both_robots(name):
    """same number of iterations, same accepted step lengths, same final (and every intermediate) regularisation; both converge within
    SolverDDP's default maxiter = 100, which is what tests/test_ik_gpu.py::test_ik_matches_numpy_ddp runs with"""
    ra, rb_ = sk.np_solve(name), sk.np_solve(name + "_absorbed")
    iters = [r["iters"] for r in ra]
    print("numpy DDP on %s: iterations %s, smallest accepted step %s" % (name, iters, [float(r["trace"][:, 2].min()) for r in ra]))
    for x, y in zip(ra, rb_):
        assert x["converged"] and y["converged"] and x["iters"] == y["iters"] <= 100
        assert np.array_equal(x["trace"][:, 1:3], y["trace"][:, 1:3]) and x["reg"] == y["reg"]
        assert rel(np.array(x["xs"]), np.array(y["xs"])) < 1e-8 and abs(x["cost"] - y["cost"]) <= 1e-9 * abs(y["cost"])
    assert len(set(iters)) > 1                        # problems of one batch finish at different iterations
