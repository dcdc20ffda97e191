"""Shared fixtures of the turning tests (tests/test_turn_cpu.py, tests/test_turn_gpu.py): the command vector, the batches of
problems.make_wb_batch with and without it, and the single-problem harness (bunmpc_amd/cyclic_gen.py :: SoloMpcGaitGen) with its
solver handles replaced by recorders.  Everything here is computed once per process and shared: do not modify what these functions
return."""
import functools
import types

import numpy as np

from bunmpc_amd import fk_np, problems
from tests import terrain_np

B = 6
W_DES = np.array([0.4, -0.3, 0.0, 0.25, -0.5, 0.0])      # mixed on purpose: rows 2 and 5 take the branch without a command
# The states of problems.make_wb_batch(model, 6, seed=SEED), chosen on the CPU: every value that is rounded to 3 decimals on the way to
# the plan (CoM xy, feet) is 1.6e-5 away from a rounding tie (seeds 1 .. 7 and the default: 4.4e-7 .. 1.6e-5; this is the largest).  The
# device's kinematics agree with numpy's to 1e-12, so every rounding falls the same way and no problem is left out of a comparison.
SEED = 3
GAITS = {"trot": (problems.TROT, problems.TROT_IK), "trot_turn": (problems.TROT_TURN, problems.TROT_TURN_IK)}
SHAPES = {"trot": (20, 10), "trot_turn": (10, 5)}          # (H, T)


def model():
    return terrain_np.solo12_model()


def stairs():
    return terrain_np.terrain("stairs", B)


@functools.lru_cache(maxsize=None)
def batch(gait, turning=True, terrain=False):
    """make_wb_batch(seed=SEED) of gait "trot" / "trot_turn", with W_DES or without a command, on flat ground or on the stairs"""
    g, ik = GAITS[gait]
    wb = problems.make_wb_batch(model(), B, seed=SEED, gait=g, ik=ik, height_map=stairs() if terrain else None, w_des=W_DES if turning else None)
    assert (wb.dyn.H, wb.ik_T) == SHAPES[gait]
    return wb


def rounded_values(x):
    """every value of the states x (B,37) that the plan builders round to 3 decimals: CoM xy (:164) and the feet (:215)"""
    kin = fk_np.kinematics(model(), x[:, :19])
    return np.concatenate([kin["com"][:, 0:2].reshape(-1), fk_np.frame_positions(model(), kin, problems.FEET).reshape(-1)])


def distance_to_rounding_tie(v):
    """how far each value is from the nearest k + 0.5 thousandths, in its own units"""
    m = np.asarray(v) * 1000.0
    return np.abs(m - np.floor(m) - 0.5) / 1000.0


def assert_away_from_ties(x):
    d = distance_to_rounding_tie(rounded_values(x)).min()
    assert d >= 1e-9, "a rounded quantity is %.3g from a tie: choose another seed" % d
    return d


def yaw_inertia():
    from bunmpc_amd.cyclic_gen import composite_inertia_base
    return float(composite_inertia_base(model(), problems.SOLO12_Q0)[2, 2])


def params(gait):
    """the gait as a BiconvexMotionParams-shaped object (motions/cyclic/solo12_trot.py)"""
    g, ik = GAITS[gait]
    return types.SimpleNamespace(
        gait_period=g.gait_period, stance_percent=list(g.stance_percent), gait_dt=g.gait_dt, phase_offset=list(g.phase_offset),
        step_ht=g.step_ht, nom_ht=g.nom_ht, gait_horizon=g.gait_horizon, W_X=g.W_X, W_X_ter=g.W_X_ter, W_F=g.W_F, rho=g.rho,
        ori_correction=list(g.ori_correction), swing_wt=list(ik["swing_wt"]), cent_wt=list(ik["cent_wt"]), reg_wt=list(ik["reg_wt"]),
        state_wt=ik["state_wt"], ctrl_wt=list(ik["ctrl_wt"]))


class Recorder:
    """stands for a solver handle: every method exists, does nothing and is written down as (name, args)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def method(*args, **kw):
            self.calls.append((name, args))
        return method


class FakeKd:
    """KinoDynMP's constructor and accessors (the pattern of tests/test_harness_gpu.py's FakeKd): no GPU behind it"""

    def __init__(self, *args):
        self.ik, self.dyn = Recorder(), Recorder()

    def set_com_tracking_weight(self, w):
        pass

    def set_mom_tracking_weight(self, w):
        pass

    def return_ik(self):
        return self.ik

    def return_dyn(self):
        return self.dyn


def host_plan(monkeypatch, gait, q, v, t, v_des_body, w, height_map=None):
    """What SoloMpcGaitGen.optimize(q, v, t, v_des_body, w) builds before it solves (abstract_cyclic_gen.py:633-656): its first lines,
    then create_cnt_plan and create_costs, on a harness whose solver handles are recorders.  Returns the harness."""
    from bunmpc_amd import cyclic_gen
    monkeypatch.setattr(cyclic_gen, "KinoDynMP", FakeKd)
    m = model()
    gg = cyclic_gen.SoloMpcGaitGen(m, m, np.concatenate([problems.SOLO12_Q0, np.zeros(18)]), 0.05, problems.SOLO12_Q0, height_map=height_map)
    gg.update_gait_params(params(gait), t)
    q = np.array(q, dtype=np.float64)
    q[0:2] = 0                                                     # :633
    ori_des = q[3:7] if w != 0 else [0, 0, 0, 1]                   # :636-639
    v_des = fk_np._quat_R(q[None, 3:7])[0] @ np.asarray(v_des_body, float)
    gg.create_cnt_plan(q, v, t, v_des, w)
    gg.create_costs(q, v, v_des, w, ori_des)
    return gg
