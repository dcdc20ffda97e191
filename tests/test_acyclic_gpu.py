"""Acyclic motions on the device (include/ext/bunmpc_acyclic.h, bunmpc_amd/acyclic_batch.py) against the twin of tests/acyclic_np.py
(SoloAcyclicGen driven with recording solver objects), the numpy DDP and the single-problem handle: Solo12 on the synthetic hop table,
B = 24 -- the twelve times of acyclic_np.TIMES with the nominal and a perturbed state --, dyn_iters = 10."""
import os

import numpy as np
import pytest

from bunmpc_amd import urdf_model
from tests import acyclic_np as twin
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
ROBOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bunmpc_amd", "robots", "solo12.json")
OUTPUTS = ("cnt_plan", "dt", "dt_ik", "x_init", "X_nom", "X_ter", "bounds", "ik_tasks", "state_w", "x_reg", "ctrl_w")
# the three problems of the anchors: in the stance (perturbed state), at the take-off (the first knots in flight) and past the table's end
ANCHORS = [2 * twin.TIMES.index((0.05, 0.0)) + 1, 2 * twin.TIMES.index((0.3, 0.0)), 2 * twin.TIMES.index((0.95, 0.0))]


@pytest.fixture(scope="module")
def model():
    return urdf_model.RobotModel.from_json(open(ROBOT).read())


@pytest.fixture(scope="module")
def hop(model):
    """the cases, the twin's arrays (computed once, never written to) and one BatchedAcyclicMpc.optimize of them"""
    import torch
    from bunmpc_amd.acyclic_batch import BatchedAcyclicMpc, DeviceAcyclicPlan
    x, t, t0 = twin.cases()
    ref = twin.plan_batch_np(model, twin.hop_plan(), x, t, t0)
    for a in ref.values():
        a.setflags(write=False)
    mpc = BatchedAcyclicMpc(model, twin.hop_plan(), dyn_iters=10)
    built = DeviceAcyclicPlan(mpc.table, len(t), x, t, t0).build().arrays()      # (a solve writes the CoM / momentum references into ik_tasks)
    out = mpc.optimize(x, t, t0)
    got = out["solver"].results()
    host = {k: out[k].cpu().numpy() for k in ("xs_int", "us_int", "f_int", "rows")}
    ptrs = {k: out[k].data_ptr() for k in ("xs_int", "us_int", "f_int", "rows", "xs", "us", "X", "F")}
    torch.cuda.synchronize()
    return dict(x=x, t=t, t0=t0, ref=ref, mpc=mpc, plan=built, got=got, host=host, ptrs=ptrs)


def check_plan(got, ref):
    for k in OUTPUTS:
        if k in ("x_init", "X_nom"):      # the entries that carry kinematics: the device's FK against numpy's
            assert np.allclose(got[k][:, :9], ref[k][:, :9], rtol=0, atol=1e-12), k
            assert np.array_equal(got[k][:, 9:], ref[k][:, 9:]), k
        else:
            assert np.array_equal(got[k], ref[k]), k


def test_plan_arrays_equal_the_twin(model, hop):
    import ctypes as C
    import torch
    from bunmpc_amd import _lib
    got, ref = hop["plan"], hop["ref"]
    check_plan(got, ref)
    assert np.all(got["status"] == 0) and np.array_equal(got["X_nom"][:, :9], got["x_init"])
    # bit for bit what the solve itself starts from
    B = len(hop["t"])
    xd, c9 = torch.from_numpy(hop["x"]).cuda(), torch.zeros((B, 9), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().bmpc_ik_centroidal_state_device(hop["mpc"].table.dm.h, C.c_void_p(xd.data_ptr()), C.c_void_p(c9.data_ptr()), B, None))
    torch.cuda.synchronize()
    assert np.array_equal(got["x_init"], c9.cpu().numpy())


def test_slot_overflow_sets_the_status_bit_and_keeps_four_tasks(model):
    from bunmpc_amd.acyclic_batch import DeviceAcyclicPlan, DeviceMotionTable
    x, t, t0 = twin.cases()
    ref = twin.plan_batch_np(model, twin.slot_plan(), x, t, t0)
    got = DeviceAcyclicPlan(DeviceMotionTable(twin.slot_plan(), model), len(t), x, t, t0).build().arrays()
    check_plan(got, ref)
    assert np.array_equal(got["status"], ref["status"]) and set(ref["status"].tolist()) == {0, twin.FRAME_SLOTS}


def test_scalar_swing_weight_means_no_swing_tasks(model):
    from bunmpc_amd.acyclic_batch import DeviceAcyclicPlan, DeviceMotionTable
    x, t, t0 = twin.cases()
    plan = twin.hop_plan()
    plan.swing_wt = 0.0
    ref = twin.plan_batch_np(model, plan, x[:12], t[:12], t0[:12])
    table = DeviceMotionTable(plan, model)
    assert table.counts["n_sw"] == 0
    check_plan(DeviceAcyclicPlan(table, 12, x[:12], t[:12], t0[:12]).build().arrays(), ref)


def test_hold_is_the_mirrors_expansion_bit_for_bit():
    """some problems with a shortened first interval, one with an empty interval, and max_rows clips the longest"""
    import torch
    from bunmpc_amd.acyclic_batch import hold_on_device
    rng = np.random.default_rng(4)
    B, n, w, size, max_rows = 9, 13, 37, 12, 595
    knots = rng.normal(size=(B, n, w))
    dt = np.full((B, 12), 0.05)
    dt[::3, 0] = 0.03
    dt[1::4, 0] = 0.02
    dt[5, 4] = 0.0
    out, rows = hold_on_device(torch.from_numpy(knots).cuda(), torch.from_numpy(dt).cuda(), size, max_rows)
    out, rows = out.cpu().numpy(), rows.cpu().numpy()
    full = [twin.hold_np(knots[b], dt[b], size).shape[0] for b in range(B)]
    assert max(full) == 600 > max_rows > min(full)
    for b in range(B):
        ref = twin.hold_np(knots[b], dt[b], size, max_rows)
        assert rows[b] == ref.shape[0] == min(full[b], max_rows)
        assert np.array_equal(out[b, :rows[b]], ref) and np.all(out[b, rows[b]:] == 0), b
    free, rows2 = hold_on_device(torch.from_numpy(knots).cuda(), torch.from_numpy(dt).cuda(), size)      # max_rows from dt
    assert free.shape[1] == 600 and np.array_equal(rows2.cpu().numpy(), full)


def test_same_inputs_same_solve(model, hop):
    """The plan built on the device, downloaded and loaded into a second plan from the host: both solves agree bit for bit -- the
    per-node strides at B > 1 -- and three problems agree with the numpy DDP on the task list rebuilt from the TWIN's arrays."""
    from bunmpc_amd.acyclic_batch import DeviceAcyclicPlan
    from oracle import ik_ddp_np
    mpc, got = hop["mpc"], hop["got"]
    B, T = len(hop["t"]), mpc.T
    second = DeviceAcyclicPlan(mpc.table, B).load_host(hop["plan"])
    kb = mpc.make_solver(second)
    kb.solve()
    again = kb.results()
    for k in ("X", "F", "xs", "us", "ik_iters"):
        assert np.array_equal(again[k], got[k]), k
    ref, names = hop["ref"], list(model.frames)
    for b in ANCHORS:
        X = got["X"][b].reshape(-1, 9)
        prob = ik_ddp_np.IKProblem(model, T)
        for t in range(T + 1):
            tk = ref["ik_tasks"][b, t]
            for sl in range(4):
                if tk[5 * sl] != 0:
                    prob._add(t, "f%d" % sl, ("frame", tk[5 * sl], (names[int(tk[5 * sl + 1])], tk[5 * sl + 2:5 * sl + 5])))
            prob._add(t, "com", ("com", tk[20], X[t, 0:3]))
            prob._add(t, "mom", ("mom", tk[24], np.concatenate([model.total_mass * X[t, 3:6], X[t, 6:9]])))
            if tk[31] != 0:
                prob._add(t, "x", ("state", tk[31], (ref["state_w"][b, t], ref["x_reg"][b, t])))
            if t < T and tk[32] != 0:
                prob._add(t, "u", ("ctrl", tk[32], ref["ctrl_w"][b, t]))
        prob.setup_costs(ref["dt_ik"][b])
        r = ik_ddp_np.solve_ddp(prob, hop["x"][b])
        err = rel_l2(got["xs"][b].reshape(-1), np.array(r["xs"]).reshape(-1))
        print("problem", b, "DDP iterations", int(got["ik_iters"][b]), r["iters"], "xs rel-L2", err)
        assert int(got["ik_iters"][b]) == r["iters"] and err < 1e-6, (b, got["ik_iters"][b], r["iters"], err)


def test_against_the_handle(model, hop):
    """the same three problems through SoloAcyclicGen.optimize (one KinoDynMP handle call each)"""
    from bunmpc_amd.acyclic_gen import SoloAcyclicGen
    got, host, plan = hop["got"], hop["host"], twin.hop_plan()
    gen = SoloAcyclicGen(model, model)
    gen.dyn_iters = 10
    for b in ANCHORS:
        x = hop["x"][b]
        gen.update_motion_params(plan, x[:19].copy(), float(hop["t0"][b]))
        xs_int, us_int, f_int = gen.optimize(x[:19].copy(), x[19:].copy(), float(hop["t"][b]))
        eX = rel_l2(got["X"][b], gen.mp.return_opt_x())
        exs = rel_l2(got["xs"][b].reshape(-1), np.array(gen.ik.get_xs()).reshape(-1))
        print("problem", b, "DDP iterations", int(got["ik_iters"][b]), gen.ik.last_stats()["iters"], "X rel-L2", eX, "xs rel-L2", exs)
        assert gen.ik.last_stats()["iters"] == got["ik_iters"][b], b
        assert eX < 1e-9 and exs < 1e-8, (b, eX, exs)
        assert host["rows"][b] == xs_int.shape[0] == us_int.shape[0] == f_int.shape[0]
        for name, ref in (("xs_int", xs_int), ("us_int", us_int), ("f_int", f_int)):      # the rows are the knots, held
            assert rel_l2(host[name][b, :host["rows"][b]].reshape(-1), ref.reshape(-1)) < 1e-7, (b, name)
    assert np.all(host["rows"] == 600)
    xs = got["xs"]
    assert np.array_equal(host["xs_int"][:, 0], xs[:, 0]) and np.array_equal(host["xs_int"][:, 49], xs[:, 0]) and np.array_equal(host["xs_int"][:, 50], xs[:, 1])


def test_a_second_call_reuses_the_tensors_and_repeats_the_result(hop):
    import torch
    mpc, got, host = hop["mpc"], hop["got"], hop["host"]
    assert np.all(got["ik_status"] == 0)
    out = mpc.optimize(torch.from_numpy(hop["x"]).cuda(), hop["t"], hop["t0"])      # device tensors are taken too
    again = out["solver"].results()
    for k in ("X", "F", "xs", "us", "ik_iters", "ik_status"):
        assert np.array_equal(again[k], got[k]), k
    for k in ("xs_int", "us_int", "f_int", "rows"):
        assert np.array_equal(out[k].cpu().numpy(), host[k]), k
    for k, p in hop["ptrs"].items():
        assert out[k].data_ptr() == p, k
    plan = out["plan"].arrays()      # rebuilt in place; the solve has filled the CoM / momentum references of the task blocks since
    refs = np.r_[21:24, 25:31]
    assert not np.all(plan["ik_tasks"][:, :, refs] == 0)
    plan["ik_tasks"][:, :, refs] = 0.0
    check_plan(plan, hop["ref"])
