"""Contact-conditioned goals on the host: the goal functions of the reference's `ISL/examples/iterative_algorithm/utils.py`
(ISL = iterative_supervised_learning) under their names and argument orders, restated on numpy alone:

    construct_contact_schedule (utils.py:104-120)   switches [ee, step, x, y, z] -> schedule (n_eff, N_total, 4), zeros after a foot's events
    ee_contact_index           (utils.py:87-102)    index of the next switch of one foot, 0 where no interval holds the time
    base_wrt_goal              (utils.py:70-85)     [steps to the contact, CoM xy minus contact xy]; sim_dt is forced to 1.0, as there
    construct_cc_goal          (utils.py:36-68)     one row per step in [start_step, end_time)
    get_estimated_com          (utils.py:187-219)   round(com(q), 3)[0:2] + i sim_dt v_des[0:2]; kinematics from a RobotModel (fk_np)

Quirks are kept: the scan runs over the zero padding too, a goal index past a foot's own events reads that padding, an index past
N_total raises IndexError, fewer than two switches raise (a list or a 1-D array has no column), and start_step > end_time raises
ValueError (start_step == end_time gives an array without rows).  tests/golden/cc_goals/cc_goals_ref.npz holds recorded outputs of the
reference's own functions; these equal them bit for bit.  The device path is bunmpc_amd/cc_goal_batch.py."""
import numpy as np

from . import fk_np


def construct_cc_goal(episode_length, n_eff, contact_schedule, com, goal_horizon=1, sim_dt=0.001, start_step=0):
    """desired_goal (end_time - start_step, 3 n_eff goal_horizon): [time to contact, x, y] per (goal step, end effector)"""
    end_time = episode_length
    for ee in range(n_eff):                      # int() at every foot, as there
        end_time = int(min(end_time, np.max(contact_schedule[ee, :, 0])))
    width = 3 * n_eff
    desired_goal = np.zeros((end_time - start_step, width * goal_horizon))
    for t in range(start_step, end_time):
        row = t - start_step
        for gh in range(goal_horizon):
            for ee in range(n_eff):
                k = ee_contact_index(t, contact_schedule[ee, :, 0]) + gh
                desired_goal[row, width * gh + 3 * ee:width * gh + 3 * ee + 3] = base_wrt_goal(t, com[row, :], contact_schedule[ee, k, :], sim_dt=sim_dt)
    return desired_goal


def base_wrt_goal(time, base_pos, goal_contact, sim_dt=0.001):
    """[goal_contact time - time (in steps: utils.py:82 sets sim_dt = 1.0), base xy - contact xy]"""
    sim_dt = 1.0
    return np.hstack((sim_dt * (goal_contact[0] - time), base_pos[:-1] - goal_contact[1:-1]))


def ee_contact_index(time, ee_contact_schedule):
    """sw + 1 for the first sw with schedule[sw] <= time < schedule[sw + 1], else 0"""
    for sw in range(len(ee_contact_schedule) - 1):
        if ee_contact_schedule[sw] <= time < ee_contact_schedule[sw + 1]:
            return sw + 1
    return 0


def construct_contact_schedule(new_contact_pos, n_eff):
    """(n_eff, number of switches, 4): each foot's [step, x, y, z] events in order, zeros behind them"""
    n = len(new_contact_pos[:, 0])
    out = np.zeros((n_eff, n, 4))
    filled = np.zeros(n_eff, int)
    for i in range(n):
        ee = int(new_contact_pos[i, 0])
        out[ee, filled[ee]:filled[ee] + 1, :] = new_contact_pos[i, 1:]
        filled[ee] += 1
    return out


def get_estimated_com(pin_robot, q0, v0, v_des, end_time, sim_dt, plan):
    """(end_time, 3): row i = [round(com(q0), 3)[0:2] + i sim_dt v_des[0:2], 0.0].  pin_robot: a RobotModel, or an object whose
    `.model` is one (the reference passes a pinocchio RobotWrapper); v0 and plan are not used, as there."""
    model = getattr(pin_robot, "model", pin_robot)
    com = np.round(fk_np.kinematics(model, np.asarray(q0, float)[None])["com"][0], 3)
    return estimated_com_rows(com, v_des, end_time, sim_dt)


def estimated_com_rows(com_rounded, v_des, end_time, sim_dt):
    vcom = np.asarray(v_des, float)[0:2]
    out = np.zeros((end_time, 3))
    for i in range(end_time):
        out[i, 0:2] = com_rounded[:2] + i * sim_dt * vcom
    return out
