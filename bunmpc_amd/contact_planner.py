"""ContactPlanner: the Raibert contact plan over a whole episode, its contact switches and the contact schedule that a
contact-conditioned policy's goals are built from (`ISL/examples/iterative_algorithm/contact_planner.py:9-256`,
ISL = iterative_supervised_learning), rebuilt on this package: kinematics from a RobotModel (fk_np) instead of pinocchio, the gait
phase from gait_planner_cpp.  Same method names, arguments and return values.  It runs on the host, one problem per call; the batch
on the device is bunmpc_amd/cc_goal_batch.py, and tests/cc_goal_np.py restates the same chain a third time.

The walk is the walk of problems.contact_plan (same Raibert rule, same round(t, 3), vtrack = v_des), with the planner's differences:
the horizon is int(20.0 episode_length sim_dt gait_horizon gait_period / gait_dt) knots, every knot is gait_dt long, v_des is used as
given (no rotation), and the hip offsets are recomputed from the current q on every call -- round(hip - com, 3), y widened by
+-0.04, R(q)^T with the full base rotation, then the yaw-only planning rotation (:94-124)."""
import numpy as np

from . import fk_np
from .gait_planner_cpp import GaitPlanner
from .goals import construct_contact_schedule


def plan_knots(plan, episode_length, sim_dt=0.001):
    """contact_planner.py:130"""
    return int(20.0 * episode_length * sim_dt * plan.gait_horizon * plan.gait_period / plan.gait_dt)


class ContactPlanner:
    def __init__(self, plan):
        self.plan = plan                                   # a problems.GaitParams, or the reference's motion plan objects
        self.eff_names = ["FL_FOOT", "FR_FOOT", "HL_FOOT", "HR_FOOT"]
        self.hip_names = ["FL_HFE", "FR_HFE", "HL_HFE", "HR_HFE"]
        self.sim_dt = .001
        self.gait_planner = GaitPlanner(plan.gait_period, np.array(plan.stance_percent), np.array(plan.phase_offset), plan.step_ht)
        self.gravity = 9.81
        self.foot_size = 0.018

    def get_end_effector_contact(self, cnt_index):
        """indices (as floats, as there) of the end effectors whose flag is 1"""
        return np.array([float(j) for j in range(len(cnt_index)) if cnt_index[j] == 1.])

    def get_switches(self, cnt_plan, start_time=0):
        """rows [ee, start_time + i gait_dt / sim_dt, x, y, 1e-3] for every foot in contact at knot i >= 1 and not at i - 1, ordered
        by knot, then foot (:35-59).  No switch: []; one switch: a 1-D array -- as there."""
        out = []
        before = self.get_end_effector_contact(cnt_plan[0, :, 0])
        for i in range(1, cnt_plan.shape[0]):
            now = self.get_end_effector_contact(cnt_plan[i, :, 0])
            for ee in now:
                if ee not in before:
                    row = np.hstack((ee, start_time + i * self.plan.gait_dt / self.sim_dt, cnt_plan[i, int(ee), 1:4]))
                    row[-1] = 1e-3
                    out = row if len(out) == 0 else np.vstack((out, row))
            before = now
        return out

    def front_end(self, pin_robot, q0):
        """(com (3,), feet (4,3), hips (4,3), unrounded; hip_off (4,2) = (R_yaw offsets[j])[0:2]) of configuration q0 (:80-124)"""
        model = getattr(pin_robot, "model", pin_robot)
        q0 = np.asarray(q0, float)
        kin = fk_np.kinematics(model, q0[None])
        com = kin["com"][0]
        feet = fk_np.frame_positions(model, kin, self.eff_names)[0]
        hips = fk_np.frame_positions(model, kin, self.hip_names)[0]
        R = kin["oR"][0][0]
        offsets = np.round(hips - com, 3)
        offsets[:, 1] += np.array([0.04, -0.04, 0.04, -0.04])
        offsets = offsets @ R                               # rows R^T offsets[j]
        yaw = np.arctan2(R[1, 0], R[0, 0])                  # matrixToRpy, roll = pitch = 0, rpyToMatrix
        c, s = np.cos(yaw), np.sin(yaw)
        self.offsets = offsets
        hip_off = np.stack([c * offsets[:, 0] - s * offsets[:, 1], s * offsets[:, 0] + c * offsets[:, 1]], axis=1)
        return com, feet, hips, hip_off

    def get_raibert_contact_plan(self, pin_robot, urdf_path, q0, v0, v_des, w_des, episode_length, start_time):
        """cnt_plan (horizon, 4, 4) [in contact?, x, y, z], swing_time (horizon, 4) (:61-234).  pin_robot: a RobotModel, or an object
        whose `.model` is one; urdf_path and v0 are not used."""
        com3, feet, _, hip_off = self.front_end(pin_robot, q0)
        return self.plan_from(com3, feet, hip_off, v_des, w_des, episode_length, start_time)

    def plan_from(self, com3, feet, hip_off, v_des, w_des, episode_length, start_time):
        plan, gp = self.plan, self.gait_planner
        com, z_height = np.round(com3[0:2], 3), com3[2]
        v_des = np.asarray(v_des, float)
        vtrack = v_des[0:2]
        horizon = plan_knots(plan, episode_length, self.sim_dt)
        cnt_plan = np.zeros((horizon, 4, 4))
        self.swing_time = np.zeros((horizon, 4))
        ang_step = 0.5 * np.sqrt(z_height / self.gravity) * vtrack
        ang_step = np.array([ang_step[1] * w_des, -(ang_step[0] * w_des)])      # np.cross(ang_step, [0, 0, w_des])[0:2] (:195)
        for i in range(horizon):
            for j in range(4):
                if i == 0:
                    cnt_plan[0, j, 0] = 1 if gp.get_phase(start_time, j) == 1 else 0
                    cnt_plan[0, j, 1:4] = np.round(feet[j], 3)
                    continue
                ft = np.round(start_time + i * plan.gait_dt, 3)
                hip_loc = com + hip_off[j] + i * plan.gait_dt * vtrack
                raibert_step = 0.5 * vtrack * plan.gait_period * plan.stance_percent[j] - 0.05 * (vtrack - v_des[0:2])
                if gp.get_phase(ft, j) == 1:
                    cnt_plan[i, j, 0] = 1
                    if cnt_plan[i - 1, j, 0] == 1:
                        cnt_plan[i, j, 1:4] = cnt_plan[i - 1, j, 1:4]
                    else:
                        cnt_plan[i, j, 1:3] = raibert_step + hip_loc + ang_step
                        cnt_plan[i, j, 3] = self.foot_size
                else:
                    per_ph = np.round(gp.get_percent_in_phase(ft, j), 3)
                    cnt_plan[i, j, 1:3] = hip_loc + ang_step if per_ph < 0.5 else hip_loc + ang_step + raibert_step
                    if per_ph - 0.5 < 0.02:
                        self.swing_time[i, j] = 1
                    cnt_plan[i, j, 3] = self.foot_size
        return cnt_plan, self.swing_time

    def get_contact_schedule(self, pin_robot, urdf_path, q0, v0, v_des, w_des, episode_length, start_time):
        """cnt_schedule (n_eff, number of switches, 4) [step, x, y, z], cnt_plan (:236-256)"""
        cnt_plan, _ = self.get_raibert_contact_plan(pin_robot, urdf_path, q0, v0, v_des, w_des, episode_length, start_time)
        new_contact_pos = self.get_switches(cnt_plan, start_time / self.sim_dt)
        return construct_contact_schedule(new_contact_pos, len(self.eff_names)), cnt_plan
