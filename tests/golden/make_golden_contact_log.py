"""Record tests/golden/contact_log/contact_log_ref.npz: inputs and outputs of the REFERENCE's own functions on small contact logs.

Run by hand, on a machine that has the reference beside this repository:

    python tests/golden/make_golden_contact_log.py <path of iterative_supervised_learning> [--out tests/golden/contact_log/contact_log_ref.npz]

It loads examples/iterative_algorithm/utils.py from its place (pinocchio, which the recorded functions never touch, is an empty stub
module) and records construct_contact_schedule and construct_cc_goal on the switches of the ten logs of
tests/contact_log_cases.py::fixture_logs (the inputs are not stored: the tests make them again, and the recorded switches and goals pin them)
(T <= 100; trot, bound and jump patterns; start_step 0 and > 0; episodes shorter than their log; goal horizons 1 and 3; one log with two
events in all, one with one, one with a foot that never lands at start_step > 0: ValueError), and quaternion_to_euler_angle on 50
quaternions.  What the recording shows about IndexError: with four feet it cannot be raised at goal horizon 3 from a step >= 0.  Two
events in all leave two feet without one, their columns' maximum is 0, end_time is 0 and there is no row to raise on; and where every
foot has an event, a foot's index is at most its count - 1 and N_total at least its count + 3, so index + gh reaches N_total only from
gh = 4 on.  The log `past_schedule` is therefore recorded at goal horizon 5 as well, where construct_cc_goal does raise it.  The switches are those of bunmpc_amd.contact_log.measured_switches: the reference's
loop (simulation.py:437-550) is inline code of its rollout functions and cannot be called.  Its edge test can: Simulation.new_ee_contact
is an unbound function of self.f_arr only, and simulation.py loads here with stub modules for its simulator imports (pybullet, the
robot wrapper, the MPC, the environment, the controller, cv2, PIL, pandas where they are absent), so it is recorded on every row of the
same logs, predecessor as the loop keeps it.  Only arrays go into the file; no test reads the reference.  (The file has a directory of
its own: tests/test_oracle_cpu.py takes every *.npz directly under tests/golden/ for a centroidal fixture.)

Per log `l<i>_`: start_step, episode_length, switches ((n, 5), n = 0 for none), new_ee (the (rows, 4) 0/1 answers of new_ee_contact per
row, as np.packbits of the flattened array), sched_raised (1: construct_contact_schedule raised), schedule; per log and horizon `l<i>_h<gh>_`: raised (0: goal recorded,
1: ValueError, 2: IndexError), goal.  quat (50, 4) as (x, y, z, w), euler (50, 3) in degrees."""
import argparse
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


class _Anything(types.ModuleType):
    """a stub module: every attribute is a class named after it"""
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def load_reference(isl):
    here = os.path.join(isl, "examples", "iterative_algorithm")
    for name in ("pinocchio", "pandas", "pybullet", "robot_properties_solo", "robot_properties_solo.solo12wrapper", "mpc", "mpc.abstract_cyclic_gen",
                 "envs", "envs.pybullet_env", "controllers", "controllers.robot_id_controller", "contact_planner", "cv2", "PIL", "torch"):
        try:
            if name in ("pinocchio", "contact_planner"):
                raise ImportError
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = _Anything(name)
    mods = {}
    for name in ("utils", "simulation"):
        spec = importlib.util.spec_from_file_location(name, os.path.join(here, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["utils"], mods["simulation"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("isl")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "contact_log", "contact_log_ref.npz"))
    args = ap.parse_args()
    utils, simulation = load_reference(args.isl)
    from bunmpc_amd import contact_log
    me = types.SimpleNamespace(f_arr=["FL_FOOT", "FR_FOOT", "HL_FOOT", "HR_FOOT"])
    out, n_eff, summary = {}, 4, []
    from tests import contact_log_cases
    cases = contact_log_cases.fixture_logs()
    for i, (name, ee_pos, com, start, length) in enumerate(cases):
        k = "l%d_" % i
        used = max(0, min(len(ee_pos), length - start))
        sw = contact_log.measured_switches(ee_pos[:used], start)
        new_ee, pre = np.zeros((used, n_eff), np.int8), np.zeros((n_eff, 3))
        for r in range(used):
            for ee in simulation.Simulation.new_ee_contact(me, ee_pos[r], pre):
                new_ee[r, int(ee)] = 1
            pre[:] = ee_pos[r]
        sched, sched_raised = np.zeros((n_eff, 0, 4)), 0
        try:
            sched = utils.construct_contact_schedule(sw, n_eff)
        except (TypeError, IndexError):
            sched_raised = 1
        for key, v in (("start_step", start), ("episode_length", length), ("switches", np.asarray(sw, float).reshape(-1, 5)),
                       ("new_ee", np.packbits(new_ee, axis=None)), ("sched_raised", sched_raised), ("schedule", sched)):
            out[k + key] = np.asarray(v)
        for gh in contact_log_cases.FIXTURE_HORIZONS.get(name, (1, 3)):
            raised, goal = 0, np.zeros((0, 0))
            if not sched_raised:
                try:
                    goal = utils.construct_cc_goal(length, n_eff, sched, com, goal_horizon=gh, sim_dt=0.001, start_step=start)
                except ValueError:
                    raised = 1
                except IndexError:
                    raised = 2
            out[k + "h%d_raised" % gh], out[k + "h%d_goal" % gh] = np.asarray(raised), goal
            summary.append((name, gh, len(np.asarray(sw, float).reshape(-1, 5)), sched_raised, raised, goal.shape))
    out["names"] = np.array([c[0] for c in cases])
    rng = np.random.default_rng(0)
    quat = rng.normal(size=(50, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    quat[0], quat[1], quat[2] = (0, 0, 0, 1), (0, np.sqrt(0.5), 0, np.sqrt(0.5)), (0, -0.8, 0, 0.7)      # identity, pitch 90, a clamped asin
    out["quat"] = quat
    out["euler"] = np.array([utils.quaternion_to_euler_angle(*(float(a) for a in q)) for q in quat])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print("%d logs -> %s (%d bytes)" % (len(cases), args.out, os.path.getsize(args.out)))
    for s in summary:
        print("  %-10s gh=%d switches=%d sched_raised=%d raised=%d goal %s" % s)


if __name__ == "__main__":
    main()
