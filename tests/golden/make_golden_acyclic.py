"""Record tests/golden/acyclic/acyclic_ref.npz: what the REFERENCE's acyclic generator hands its solver objects, on its own motion tables.

Run by hand, on a machine that has the reference beside this repository:

    python tests/golden/make_golden_acyclic.py <directory that holds iterative_supervised_learning and robot_properties_solo> [--out FILE]

It loads examples/mpc/abstract_acyclic_gen.py, examples/motions/weight_abstract.py and the tables examples/motions/acyclic/{plan_jump,
rearing, rearing_jump, plan_cartwheel, plan_hifive, stand}.py from their place, under stub modules: pinocchio (utils.zero,
computeTotalMass = the mass of bunmpc_amd/robots/solo12.json, centerOfMass and data.hg from oracle/rbd_np.py, the rest no-ops),
inverse_kinematics_cpp, matplotlib, robot_properties_solo.config (Solo12Config.initial_configuration is READ from the reference's
robot_properties_solo/src/robot_properties_solo/config.py, as text, and evaluated; getFrameId(name) is the frame's index in solo12.json)
and biconvex_mpc_cpp, whose KinoDynMP is the recording object of tests/acyclic_np.py (_Kd).  Only arrays go into the file, never the
reference's text, and no test reads the reference: the tests rebuild every table from the file alone (acyclic_np.unpack_table).

Recorded
  q0, q0_is_SOLO12_Q0           Solo12Config.initial_configuration and whether it equals problems.SOLO12_Q0 (it does not: the reference
                                stands at x = 0.2, z = 0.25)
  <table>__<field>              every field of the five usable tables (acyclic_np.pack_table: lists with a row count, swing_wt as a flag)
  stand_raised, stand_error     `stand` has no plan_freq: update_motion_params raises, and only that is recorded
  <table>__x, t, t0             the cases: the times of acyclic_np.TIMES; every boundary of the contact phases and the boundary +- 0.01;
                                t - t0 at the table's end and beyond it; one off-grid absolute t with t0 != 0; two times whose fourth
                                decimal is 5 (np.round(., 3) decides on the binary value).  The perturbed state of acyclic_np.states() at
                                every time, the nominal one at three; and at PLACED_TIMES the perturbed state moved to where the
                                reference starts (its base position + q0[:3] - SOLO12_Q0[:3]): the twin's states stand 0.2 m behind
                                the tables' contact locations, where the centroidal ADMM is in its chaotic regime or diverges on
                                most cases (tests/test_acyclic_ref_cpu.py measures that), so no solve can be compared on them.
  <table>__state_kind           per case: acyclic_np.STATE_NOMINAL, STATE_PERTURBED or STATE_PLACED
  <table>__x_init               the centroidal state handed to the reference through the pinocchio stub -- an INPUT of the recording,
                                computed by oracle/rbd_np.py, NOT the reference's (pinocchio is not here)
  <table>__out_<array>          what create_contact_plan / create_costs passed to the solver objects, in the layout of acyclic_np.plan_np:
                                cnt_plan, dt, dt_ik, X_nom (its first nine entries are x_init), X_ter, bounds, ik_tasks, state_w, x_reg,
                                ctrl_w, and frames, the frame-task count per node
  <table>__size                 update_motion_params' size
  <table>__grid, freq, gains    get_plan_freq and get_gains on 30 times from before t0 to past the table's end (plan_jump, rearing; NaN
                                where the reference returns None)
  <table>__hold_*               the reference's own expansion (optimize :331-345) at two times, with a solver stub whose optimize does
                                nothing and whose return_opt_f / get_xs / get_us return seeded arrays: the knots xs, us, F, the dt array
                                and xs_int, us_int, f_int.  The dt array the reference expands with is the self.dt_arr that create_costs
                                fills from params.dt_arr (n_col entries and a last 0), not the contact plan's shortened first-knot dt.
  hold_edge_knots, _dt, _rows, _out   acyclic_np.hold_edge_problems and hold_np's expansion of them (rows past a problem's own are 0): the
                                intervals k ms with int((k / 1000) / 0.001) == k - 1, asserted below for every k of acyclic_np.HOLD_EDGES_MS"""
import argparse
import ast
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HOLD_TIMES = ((0.02, 0.0), (0.6, 0.0))
PLACED_TIMES = ((0.05, 0.0), (0.88, 0.0), (1.5, 0.0))
GRID_TABLES = ("plan_jump", "rearing")


def initial_configuration(ref):
    """Solo12Config.initial_configuration, read from the reference's config.py without importing it (it needs pinocchio and the URDFs)"""
    path = os.path.join(ref, "robot_properties_solo", "src", "robot_properties_solo", "config.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Solo12Config")
    node = next(n for n in cls.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "initial_configuration")
    return np.array(eval(compile(ast.Expression(node.value), path, "eval"), {}), dtype=np.float64)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref, model, q0):
    """(the generator's module, {table name: plan or the exception its file raised}) under the stubs of the docstring"""
    from oracle import rbd_np
    from tests import acyclic_np as twin
    isl = os.path.join(ref, "iterative_supervised_learning", "examples")
    rmodel = types.SimpleNamespace(nq=model.nq, nv=model.nv, getFrameId=model.frame_id)
    robot = types.SimpleNamespace(model=rmodel, data=types.SimpleNamespace(hg=np.zeros(6)))

    def center_of_mass(rm, rdata, q, v):
        kin = rbd_np.Kin(model, q, v)
        rdata.hg = kin.centroidal_momentum()
        return kin.com

    nothing = lambda *a, **k: None      # noqa: E731
    pin = types.ModuleType("pinocchio")
    pin.utils = types.SimpleNamespace(zero=np.zeros)
    pin.computeTotalMass, pin.centerOfMass = (lambda rm: model.total_mass), center_of_mass
    pin.computeCentroidalMomentum = pin.forwardKinematics = pin.updateFramePlacements = pin.framesForwardKinematics = nothing
    made = []

    def kino_dyn_mp(urdf, m, n_eff, horizon, ik_horizon):
        assert horizon == ik_horizon and n_eff == 4 and m == model.total_mass
        made.append(twin._Kd(ik_horizon))
        return made[-1]

    config = types.ModuleType("robot_properties_solo.config")
    config.Solo12Config = types.SimpleNamespace(initial_configuration=q0.tolist(), buildRobotWrapper=lambda: robot)
    stubs = {"pinocchio": pin, "inverse_kinematics_cpp": types.SimpleNamespace(InverseKinematics=None),
             "biconvex_mpc_cpp": types.SimpleNamespace(KinoDynMP=kino_dyn_mp), "matplotlib": types.SimpleNamespace(pyplot=None),
             "matplotlib.pyplot": types.ModuleType("matplotlib.pyplot"), "robot_properties_solo": types.ModuleType("robot_properties_solo"),
             "robot_properties_solo.config": config, "motions": types.ModuleType("motions")}
    saved = {k: sys.modules.get(k) for k in list(stubs) + ["motions.weight_abstract"]}
    sys.modules.update(stubs)
    try:
        _load("motions.weight_abstract", os.path.join(isl, "motions", "weight_abstract.py"))
        gen = _load("_ref_abstract_acyclic_gen", os.path.join(isl, "mpc", "abstract_acyclic_gen.py"))
        plans = {name: _load("_ref_motion_" + name, os.path.join(isl, "motions", "acyclic", name + ".py")).plan for name in twin.REF_TABLES + ("stand",)}
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return gen, robot, made, plans


def case_times(plan):
    """the (t, t0) of one table, each once, in the docstring's order; and the three at which the nominal state is recorded too"""
    from tests import acyclic_np as twin
    edges = sorted({float(row[0][c]) for row in plan.cnt_plan for c in (4, 5)})
    end = edges[-1]
    times = list(twin.TIMES)
    times += [(float(np.round(e + d, 2)), 0.0) for e in edges for d in (0.0, -0.01, 0.01)]
    times += [(end + 0.3, 0.3), (end + 0.37, 0.0), (0.613, 0.25), (0.4125, 0.0), (0.2375, 0.0)]
    once = []
    for tt in times:
        if tt not in once:
            once.append(tt)
    return once, [twin.TIMES[0], twin.TIMES[5], (end + 0.3, 0.3)]


def record(ref):
    from bunmpc_amd import problems, urdf_model
    from tests import acyclic_np as twin
    model = urdf_model.RobotModel.from_json(open(os.path.join(ROOT, "bunmpc_amd", "robots", "solo12.json")).read())
    q0 = initial_configuration(ref)
    gen_mod, robot, made, plans = load_reference(ref, model, q0)
    out = dict(q0=q0, q0_is_SOLO12_Q0=np.int64(np.array_equal(q0, problems.SOLO12_Q0)), tables=np.array(twin.REF_TABLES))
    summary = []
    states = twin.states()

    def generator(plan, x, t0):
        gen = gen_mod.SoloAcyclicGen(robot, None)
        gen.update_motion_params(plan, x[:19].copy(), float(t0))
        return gen, made[-1]

    # stand: no plan_freq
    try:
        generator(plans["stand"], states[0], 0.0)
        out["stand_raised"], out["stand_error"] = np.int64(0), np.array("")
    except Exception as e:      # noqa: BLE001 -- whatever it is, its name is what is recorded
        out["stand_raised"], out["stand_error"] = np.int64(1), np.array(type(e).__name__)
    for name in twin.REF_TABLES:
        plan = plans[name]
        for k, v in twin.pack_table(plan).items():
            out["%s__%s" % (name, k)] = v
        times, nominal = case_times(plan)
        placed = states[1].copy()
        placed[:3] += q0[:3] - problems.SOLO12_Q0[:3]
        cases = ([(states[1], t, t0, twin.STATE_PERTURBED) for t, t0 in times] + [(states[0], t, t0, twin.STATE_NOMINAL) for t, t0 in nominal] +
                 [(placed, t, t0, twin.STATE_PLACED) for t, t0 in PLACED_TIMES])
        rows = []
        for x, t, t0, kind in cases:
            gen, kd = generator(plan, x, t0)
            gen.create_contact_plan(x[:19].copy(), x[19:].copy(), float(t))
            gen.create_costs(x[:19].copy(), x[19:].copy(), float(t))
            H = plan.n_col
            tasks = kd.ik.tasks
            tasks[:, 20], tasks[:, 24] = kd.wt_com, kd.wt_mom      # as plan_np: the tracking weights of every node
            assert len(kd.mp.cnt) == H and kd.ik.dt.shape == (H + 1,) and kd.ik.dt[H] == 0
            rows.append(dict(x=x, t=t, t0=t0, state_kind=kind, x_init=kd.mp.X_nom[0:9].copy(), size=gen.size, out_cnt_plan=np.array(kd.mp.cnt), out_dt=np.array(kd.mp.dt),
                             out_dt_ik=kd.ik.dt[:H].copy(), out_X_nom=kd.mp.X_nom, out_X_ter=kd.mp.X_ter, out_bounds=kd.mp.bounds, out_ik_tasks=tasks,
                             out_state_w=kd.ik.state_w, out_x_reg=kd.ik.x_reg, out_ctrl_w=kd.ik.ctrl_w, out_frames=np.array(kd.ik.frames)))
        for k in rows[0]:
            out["%s__%s" % (name, k)] = np.stack([np.asarray(r[k]) for r in rows])
        if name in GRID_TABLES:
            t0 = 0.22
            gen, _ = generator(plan, states[0], t0)
            grid = t0 + np.linspace(-0.1, float(plan.cnt_plan[-1][0][5]) + 0.3, 30)
            nan = lambda v: np.nan if v is None else float(v)      # noqa: E731
            out[name + "__grid"], out[name + "__grid_t0"] = grid, np.float64(t0)
            out[name + "__freq"] = np.array([nan(gen.get_plan_freq(float(t))) for t in grid])
            out[name + "__gains"] = np.array([[nan(v) for v in (gen.get_gains(float(t)) or (None, None))] for t in grid])
        # the reference's own expansion
        T = plan.n_col
        hold = []
        for j, (t, t0) in enumerate(HOLD_TIMES):
            rng = np.random.default_rng([331, twin.REF_TABLES.index(name), j])
            xs, us, F = rng.normal(size=(T + 1, 37)), rng.normal(size=(T, 18)), rng.normal(size=12 * T)
            gen, kd = generator(plan, states[1], t0)
            kd.optimize = lambda q, v, iters, flag: None
            kd.mp.return_opt_f, kd.ik.get_xs, kd.ik.get_us = (lambda F=F: F), (lambda xs=xs: xs), (lambda us=us: us)
            with contextlib.redirect_stdout(io.StringIO()):
                xs_int, us_int, f_int = gen.optimize(states[1][:19].copy(), states[1][19:].copy(), float(t))
            hold.append(dict(hold_t=t, hold_t0=t0, hold_xs=xs, hold_us=us, hold_F=F.reshape(T, 12), hold_dt=np.array(gen.dt_arr), hold_xs_int=xs_int,
                             hold_us_int=us_int, hold_f_int=f_int))
        for k in hold[0]:
            out["%s__%s" % (name, k)] = np.stack([np.asarray(h[k]) for h in hold])
        summary.append((name, len(cases), T, int(max(r["out_frames"].max() for r in rows)), out[name + "__hold_xs_int"].shape))
    # the hold's edge intervals
    for k in twin.HOLD_EDGES_MS:
        assert int((k / 1000) / 0.001) == k - 1, k
    assert int(0.04 / 0.001) == 40 and int(0.05 / 0.001) == 50
    knots, dt = twin.hold_edge_problems()
    full = [twin.hold_np(knots[b], dt[b], 12) for b in range(len(dt))]
    rows = np.array([len(f) for f in full])
    expanded = np.zeros((len(dt), rows.max(), 37))
    for b, f in enumerate(full):
        expanded[b, :len(f)] = f
    out.update(hold_edge_knots=knots, hold_edge_dt=dt, hold_edge_rows=rows, hold_edge_out=expanded)
    return out, summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "acyclic", "acyclic_ref.npz"))
    args = ap.parse_args()
    out, summary = record(args.reference)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print("%s (%d bytes); q0 is SOLO12_Q0: %d; stand raised %s" % (args.out, os.path.getsize(args.out), out["q0_is_SOLO12_Q0"], out["stand_error"]))
    for s in summary:
        print("  %-15s cases=%d n_col=%d most frame tasks at a node=%d xs_int %s" % s)


if __name__ == "__main__":
    main()
