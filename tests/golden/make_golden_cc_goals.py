"""Record tests/golden/cc_goals/cc_goals_ref.npz: inputs and outputs of the REFERENCE's own goal functions.

Run by hand, on a machine that has the reference beside this repository:

    python tests/golden/make_golden_cc_goals.py <path of iterative_supervised_learning> [--out tests/golden/cc_goals/cc_goals_ref.npz]

It loads examples/iterative_algorithm/utils.py and contact_planner.py from their place.  Their imports that the goal code never
touches -- pinocchio, gait_planner_cpp, mpc.abstract_cyclic_gen -- are stubbed with empty modules, and ContactPlanner is made with
object.__new__ (its constructor builds a GaitPlanner), so get_switches runs as written.  get_estimated_com asks pinocchio for the
centre of mass and for nothing else: the stub's centerOfMass returns the CoM of the case, forwardKinematics / updateFramePlacements do
nothing, and what is recorded is the reference's arithmetic on that CoM (rounding, the row loop).  The contact plans that go in are
40-knot plans of problems.contact_plan.  Only arrays go into the file; no test reads the reference.  (The file has a directory of its
own: tests/test_oracle_cpu.py takes every *.npz directly under tests/golden/ for a centroidal fixture.)

Per plan `p<i>_`: cnt_plan, start (get_switches' start_time, in steps), switches, schedule, com3, v_des, index_t, index
(ee_contact_index of every foot at the steps index_t); per case `c<i>_`: plan, goal_length (construct_cc_goal's episode_length),
goal_horizon, start_step, est_com (get_estimated_com's rows up to five past the goal's, of goal_length), raised (0: goal recorded,
1: ValueError, 2: IndexError), goal."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def load_reference(isl):
    pin = types.ModuleType("pinocchio")
    pin.forwardKinematics = lambda *a: None
    pin.updateFramePlacements = lambda *a: None
    pin.centerOfMass = lambda model, data, q, v: np.array(model.com, float)
    sys.modules["pinocchio"] = pin
    gp = types.ModuleType("gait_planner_cpp")
    gp.GaitPlanner = object
    sys.modules["gait_planner_cpp"] = gp
    mpc = types.ModuleType("mpc")
    acg = types.ModuleType("mpc.abstract_cyclic_gen")
    acg.SoloMpcGaitGen = object
    sys.modules["mpc"], sys.modules["mpc.abstract_cyclic_gen"] = mpc, acg
    here = os.path.join(isl, "examples", "iterative_algorithm")
    mods = {}
    for name in ("utils", "contact_planner"):
        spec = importlib.util.spec_from_file_location(name, os.path.join(here, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["utils"], mods["contact_planner"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("isl")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cc_goals", "cc_goals_ref.npz"))
    args = ap.parse_args()
    utils, cp = load_reference(args.isl)
    from bunmpc_amd import problems

    out, case, n_eff, H = {}, 0, 4, 40
    plans = [(problems.TROT, 0.0), (problems.TROT, 0.13), (problems.BOUND, 0.0), (problems.BOUND, 0.2), (problems.JUMP, 0.0), (problems.JUMP, 0.37)]
    for p, (gait, t0) in enumerate(plans):
        com3 = np.array([0.0123 + 0.01 * p, -0.0071, 0.231])
        v_des, w_des = np.array([0.3, 0.1 - 0.05 * p, 0.0]), 0.2
        feet0 = np.round(np.c_[problems.SOLO12.feet_xy, np.full(4, 0.018)], 3)
        cnt, _, _ = problems.contact_plan(gait, problems.SOLO12, H, np.array([t0]), np.round(com3[None, 0:2], 3), com3[None, 2], feet0[None],
                                          v_des[None], np.array([w_des]))
        planner = object.__new__(cp.ContactPlanner)
        planner.plan, planner.sim_dt = types.SimpleNamespace(gait_dt=gait.gait_dt), .001
        start = t0 / planner.sim_dt
        sw = planner.get_switches(cnt[0], start)
        sched = utils.construct_contact_schedule(sw, n_eff)
        last = min(int(np.max(sched[ee, :, 0])) for ee in range(n_eff))
        first = int(np.ceil(np.min(sw[:, 1])))
        second = int(np.sort(sw[:, 1])[len(sw) // 2])
        index_t = np.arange(int(start) - 2, int(np.max(sw[:, 1])) + 60)
        out["p%d_index_t" % p] = index_t
        out["p%d_index" % p] = np.array([[utils.ee_contact_index(t, sched[ee, :, 0]) for t in index_t] for ee in range(n_eff)])
        for name, v in (("cnt_plan", cnt[0]), ("start", start), ("switches", sw), ("schedule", sched), ("com3", com3), ("v_des", v_des)):
            out["p%d_%s" % (p, name)] = np.asarray(v)
        robot = types.SimpleNamespace(model=types.SimpleNamespace(com=com3), data=None)
        # (goal_length, start_step, goal horizons): before the first event, between events, up to the end of the schedule (where
        # the extra goal steps read the zero padding), after a foot's last event (raises), a goal horizon past N_total (raises)
        kinds = [(int(start) + 80, int(start), (1, 2, 3)), (second + 60, second + 3, (1, 2, 3)), (3001, last - 40, (1, 2, 3)),
                 (3001, last + 5, (1,)), (3001, last - 10, (len(sw),)), (first + 30, max(first - 5, 0), (2,))]
        for goal_length, start_step, horizons in kinds:
            est = utils.get_estimated_com(robot, None, None, v_des, goal_length, planner.sim_dt, None)
            for gh in horizons:
                k = "c%d_" % case
                raised, goal = 0, np.zeros((0, 0))
                try:
                    goal = utils.construct_cc_goal(goal_length, n_eff, sched, est, goal_horizon=gh, sim_dt=planner.sim_dt, start_step=start_step)
                except ValueError:
                    raised = 1
                except IndexError:
                    raised = 2
                for name, v in (("goal_length", goal_length), ("goal_horizon", gh), ("start_step", start_step), ("est_com", est[:goal.shape[0] + 5]),
                                ("raised", raised), ("goal", goal), ("plan", p)):
                    out[k + name] = np.asarray(v)
                case += 1
    out["n_cases"], out["n_plans"] = np.asarray(case), np.asarray(len(plans))
    np.savez_compressed(args.out, **out)
    print("%d cases of %d plans -> %s (%d bytes)" % (case, len(plans), args.out, os.path.getsize(args.out)))
    raised = [int(out["c%d_raised" % i]) for i in range(case)]
    print("raised:", {r: raised.count(r) for r in set(raised)}, "rows:", sorted({out["c%d_goal" % i].shape[0] for i in range(case)}))
    pads = 0
    for i in range(case):
        if raised[i] == 0 and int(out["c%d_goal_horizon" % i]) > 1:
            pads += int(np.any(out["c%d_goal" % i][:, 12] == -np.arange(int(out["c%d_start_step" % i]), int(out["c%d_start_step" % i]) + out["c%d_goal" % i].shape[0])))
    print("cases with a slot that reads the zero padding:", pads)


if __name__ == "__main__":
    main()
