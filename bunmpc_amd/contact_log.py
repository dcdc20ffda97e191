"""Measured contact goals: the contacts logged during rollouts turned into the cc_goals rows of the data set, as the reference's data
collection does after its simulator has stepped (`ISL/examples/iterative_algorithm/simulation.py:537-550` with `:563-578`, and the same
block in three more rollout functions; ISL = iterative_supervised_learning).  The simulator is not here; the block that turns its
measurements into goals is array code on a log, and anyone with logged rollouts has its inputs: `ee_pos` (T, 4, 3) per step, and `q`, `v`.

Host, one episode, restated on numpy alone under the reference's semantics (quirks kept; tests/golden/contact_log/contact_log_ref.npz
holds recorded outputs of the reference's own functions):

    rising_feet        (simulation.py:299-314)   feet whose |x| rose above 1e-12 from a predecessor at or below it
    measured_switches  (simulation.py:437-550)   what the loop leaves in new_contact_pos: [], one entry (5,), or (n, 5) [ee, o, x, y, z]
    measured_cc_goals  (simulation.py:563-568)   goals.construct_contact_schedule + goals.construct_cc_goal on them; raises where they raise
    quaternion_to_euler_angle (utils.py:7-34),  failed_states (simulation.py:189-220)
    host_batch         the device call's twin: B episodes, statuses in place of exceptions, the arrays of bunmpc_contact_log.h

Device: `DeviceContactLog` (include/ext/bunmpc_contact_log.h, csrc/contact_log.hip) builds goals, rows, status, schedule, counts and
failed_step of B logged episodes in HBM; `episode_groups` makes states, vc_goals and the CoM rows from logged q, v with the kernels the
data path already has; `DeviceDatabase.append_episodes` takes the result.  Nothing leaves the device."""
import ctypes as C
import math

import numpy as np

from . import goals

THRESHOLD = 1e-12      # simulation.py:310


# ---- host: one episode -------------------------------------------------------------------------------------------------------------------

def rising_feet(row, before):
    """feet j, ascending, with |row[j][0]| above the threshold and |before[j][0]| at or below it: only x is looked at, and both
    comparisons are written this way round, so a NaN is neither a contact nor a cleared predecessor (simulation.py:299-314)"""
    return [j for j in range(len(row)) if abs(row[j][0]) > THRESHOLD and abs(before[j][0]) <= THRESHOLD]


def measured_switches(ee_pos_log, start_step):
    """ee_pos_log (rows, 4, 3): the contact positions of steps start_step, start_step + 1, ... (zeros for a foot in the air).  One event
    [foot, step, x, y, z] per foot that rises at a row, rows ascending and feet ascending within a row; the predecessor is zeros before
    row 0 and the row itself afterwards, recorded or not; nothing is recorded at step 0 (the absolute step, whatever the row).  Returns
    what the reference's loop leaves behind (simulation.py:437-550): [] without an event, one (5,) array with one, (n, 5) otherwise."""
    log = np.asarray(ee_pos_log, float)
    events, before = [], np.zeros(log.shape[1:])
    for r, row in enumerate(log):
        step = start_step + r
        if step != 0:
            events += [np.concatenate(([float(j), float(step)], row[j])) for j in rising_feet(row, before)]
        before = row
    if not events:
        return []
    return events[0] if len(events) == 1 else np.array(events)


def measured_cc_goals(ee_pos_log, com_log, episode_length, start_step, goal_horizon=1, n_eff=4):
    """(schedule, cc_goal_history) of one logged episode: the rows of range(start_step, episode_length) that the log holds, their
    switches, the schedule and the goals over the measured CoM rows com_log (rows, 3).  Raises what the reference raises: with fewer
    than two switches (a list or a 1-D array has no column), IndexError past the schedule, ValueError where start_step > end_time."""
    rows = max(0, min(len(ee_pos_log), episode_length - start_step))
    switches = measured_switches(np.asarray(ee_pos_log, float)[:rows], start_step)
    schedule = goals.construct_contact_schedule(switches, n_eff)
    return schedule, goals.construct_cc_goal(episode_length, n_eff, schedule, np.asarray(com_log, float), goal_horizon=goal_horizon, start_step=start_step)


def quaternion_to_euler_angle(x, y, z, w):
    """(roll, pitch, yaw) in degrees of the unit quaternion (x, y, z, w), ZYX angles with the sine of the pitch clamped to [-1, 1]; the
    operations and their order are those of utils.py:7-34, which the recorded angles need"""
    yy = y * y
    sin_pitch = 2.0 * (w * y - z * x)
    if sin_pitch > 1.0:
        sin_pitch = 1.0
    elif sin_pitch < -1.0:
        sin_pitch = -1.0
    roll = math.atan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + yy))
    yaw = math.atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (yy + z * z))
    return math.degrees(roll), math.degrees(math.asin(sin_pitch)), math.degrees(yaw)


def failed_states(q, time_elapsed, gait_period, sim_dt, lax, fail_angle=30):
    """True once the rows of one gait period have passed (time_elapsed > gait_period / sim_dt) and the base is below z_min (0.05 with
    `lax`, for jump and bound; 0.1 otherwise), above 2.0, or rolled or pitched by more than fail_angle degrees; every comparison is
    strict (simulation.py:189-220)"""
    if not time_elapsed > gait_period / sim_dt:
        return False
    roll, pitch, _ = quaternion_to_euler_angle(float(q[3]), float(q[4]), float(q[5]), float(q[6]))
    z_min = 0.05 if lax else 0.1
    return bool(q[2] < z_min or q[2] > 2.0 or abs(roll) > fail_angle or abs(pitch) > fail_angle)


# ---- host: the device call's twin ---------------------------------------------------------------------------------------------------------

FEW_SWITCHES, START_AFTER_END, PAST_SCHEDULE, EVENTS_OVERFLOW, FAILED_STATE = 1, 2, 4, 8, 16      # include/ext/bunmpc_contact_log.h


def _leading_rows(episode_length, n_eff, schedule, com, goal_horizon, start_step):
    """construct_cc_goal row by row: (rows before the first IndexError, 12 goal_horizon), whether one was raised"""
    end_time = episode_length
    for ee in range(n_eff):
        end_time = int(min(end_time, np.max(schedule[ee, :, 0])))
    out = []
    for t in range(start_step, end_time):
        row = np.zeros(3 * n_eff * goal_horizon)
        try:
            for gh in range(goal_horizon):
                for ee in range(n_eff):
                    k = goals.ee_contact_index(t, schedule[ee, :, 0]) + gh
                    row[3 * n_eff * gh + 3 * ee:3 * n_eff * gh + 3 * ee + 3] = goals.base_wrt_goal(t, com[t - start_step, :], schedule[ee, k, :])
        except IndexError:
            return np.array(out).reshape(len(out), 3 * n_eff * goal_horizon), True
        out.append(row)
    return np.array(out).reshape(len(out), 3 * n_eff * goal_horizon), False


def host_batch(ee_pos, com, start_step, episode_length, goal_horizon=1, max_events=64, max_rows=None, q=None, z_min=0.1, fail_angle=30.0,
               grace=0.0):
    """What bmpc_contact_log_goals_device leaves, through the host functions above: ee_pos (B, T, 4, 3), com (B, T, 3), start_step (B,),
    q (B, T, >= 19) or None.  Returns a dict of goals (B, max_rows, 12 goal_horizon), rows, status, schedule (B, 4, max_events, 4), counts,
    failed_step and angles (B, T, 2; NaN without q)."""
    ee_pos, com = np.asarray(ee_pos, float), np.asarray(com, float)
    B, T, n_eff = ee_pos.shape[0], ee_pos.shape[1], 4
    max_rows = T if max_rows is None else max_rows
    out = dict(goals=np.zeros((B, max_rows, 3 * n_eff * goal_horizon)), rows=np.zeros(B, np.int32), status=np.zeros(B, np.int32),
               schedule=np.zeros((B, n_eff, max_events, 4)), counts=np.zeros((B, n_eff), np.int32), failed_step=np.full(B, -1, np.int32),
               angles=np.full((B, T, 2), np.nan))
    for b in range(B):
        start = int(start_step[b])
        used = max(0, min(T, episode_length - start))
        sw = measured_switches(ee_pos[b, :used], start)
        sw2 = np.asarray(sw, float).reshape(-1, 5)
        for j in range(n_eff):
            mine = sw2[sw2[:, 0] == j][:, 1:]
            out["counts"][b, j] = len(mine)
            out["schedule"][b, j, :min(len(mine), max_events)] = mine[:max_events]
        status, rows = 0, 0
        if len(sw2) > max_events:
            status = EVENTS_OVERFLOW
        else:
            try:
                schedule = goals.construct_contact_schedule(sw, n_eff)
            except (TypeError, IndexError):      # a list, or a 1-D array, has no column
                schedule, status = None, FEW_SWITCHES
            if schedule is not None:
                assert np.array_equal(schedule, out["schedule"][b, :, :len(sw2)], equal_nan=True)
                end_time = episode_length
                for ee in range(n_eff):
                    end_time = int(min(end_time, np.max(schedule[ee, :, 0])))
                if start > end_time:                 # np.zeros of a negative number of rows: ValueError
                    status = START_AFTER_END
                else:
                    g, raised = _leading_rows(episode_length, n_eff, schedule, com[b], goal_horizon, start)
                    status = PAST_SCHEDULE if raised else 0
                    rows = min(len(g), max_rows)
                    out["goals"][b, :rows] = g[:rows]
        if q is not None:
            for r in range(T):
                rpy = quaternion_to_euler_angle(*(float(a) for a in q[b, r, 3:7]))
                out["angles"][b, r] = rpy[0:2]
                if r < used and out["failed_step"][b] < 0 and r > grace and (
                        q[b, r, 2] < z_min or q[b, r, 2] > 2.0 or abs(rpy[0]) > fail_angle or abs(rpy[1]) > fail_angle):
                    out["failed_step"][b] = r
            if out["failed_step"][b] >= 0:
                status, rows = status | FAILED_STATE, 0
                out["goals"][b] = 0.0
        out["rows"][b], out["status"][b] = rows, status
    return out


# ---- device ------------------------------------------------------------------------------------------------------------------------------

def default_max_events(T):
    """room for a touchdown of every foot each 100 steps, plus two per foot for the ends"""
    return max(8, 4 * (int(T) // 100 + 2))


class DeviceContactLog:
    """goals (B, max_rows, 12 goal_horizon) with zeros from row rows[b] on, rows, status (the BMPC_CL_* bits), schedule
    (B, 4, max_events, 4), counts (B, 4), failed_step (B,) and, with want_angles, angles (B, T, 2) as device tensors, allocated once and
    written again by every build()."""

    def __init__(self, B, T, goal_horizon=1, max_events=None, max_rows=None, want_angles=False, device="cuda"):
        import torch
        from . import _lib_contact_log
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceContactLog needs a GPU")
        self.torch, self.device = torch, torch.device(device)
        self.B, self.T, self.goal_horizon = int(B), int(T), int(goal_horizon)
        self.max_events = default_max_events(T) if max_events is None else int(max_events)
        self.max_rows = self.T if max_rows is None else int(max_rows)
        f64, i32 = dict(dtype=torch.float64, device=self.device), dict(dtype=torch.int32, device=self.device)
        self.goals = torch.empty((self.B, self.max_rows, 12 * self.goal_horizon), **f64)
        self.rows, self.status, self.failed_step = torch.empty(self.B, **i32), torch.empty(self.B, **i32), torch.empty(self.B, **i32)
        self.schedule, self.counts = torch.empty((self.B, 4, self.max_events, 4), **f64), torch.empty((self.B, 4), **i32)
        self.angles = torch.empty((self.B, self.T, 2), **f64) if want_angles else None
        d = _lib_contact_log.ContactLog()
        d.B, d.T, d.n_eff, d.goal_horizon, d.max_events, d.max_rows = self.B, self.T, 4, self.goal_horizon, self.max_events, self.max_rows
        for k in ("goals", "rows", "status", "failed_step", "schedule", "counts", "angles"):
            t = getattr(self, k)
            setattr(d, k, t.data_ptr() if t is not None and t.numel() else None)
        self.desc, self._lib = d, _lib_contact_log

    def _input(self, name, t, shape, dtype):
        torch = self.torch
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.ascontiguousarray(t))
        t = t.to(device=self.device, dtype=dtype)
        if tuple(t.shape) != shape:
            raise ValueError("%s: expected shape %s, got %s" % (name, shape, tuple(t.shape)))
        return t

    def build(self, ee_pos, com, start_step, episode_length, q=None, z_min=None, fail_angle=30, gait_period=None, sim_dt=0.001):
        """ee_pos (B, T, 4, 3), com (B, T, 3), start_step (B,) = int(start_time / sim_dt); q (B, T, 19) -- a view of rows [q, v] is passed
        in place -- switches the failed-state test on and needs gait_period (the test starts after row gait_period / sim_dt); z_min: 0.05
        for jump and bound, 0.1 (the default) otherwise.  Asynchronous on torch's current stream."""
        from . import _lib
        torch, d, B, T = self.torch, self.desc, self.B, self.T
        hold = [self._input("ee_pos", ee_pos, (B, T, 4, 3), torch.float64).contiguous(), self._input("com", com, (B, T, 3), torch.float64).contiguous(),
                self._input("start_step", start_step, (B,), torch.int32).contiguous()]
        d.episode_length, d.check_failed = int(episode_length), int(q is not None)
        d.z_min, d.fail_angle, d.grace, d.q, d.s_q = 0.1 if z_min is None else float(z_min), float(fail_angle), 0.0, None, 0
        if q is not None:
            if gait_period is None:
                raise ValueError("the failed-state test needs gait_period")
            q = self._input("q", q, (B, T, 19), torch.float64)
            if B and (q.stride(2) != 1 or q.stride(1) < 19 or (B > 1 and q.stride(0) != T * q.stride(1))):
                q = q.contiguous()
            hold.append(q)
            d.grace, d.s_q = float(gait_period) / float(sim_dt), q.stride(1) if B else 19
        if B == 0:
            return self
        d.ee_pos, d.com, d.start_step = (t.data_ptr() for t in hold[:3])
        if q is not None:
            d.q = q.data_ptr()
        # (`hold` keeps converted copies alive until the kernels are enqueued; freed after that, their memory is reused in stream order)
        _lib.check(self._lib.lib().bmpc_contact_log_goals_device(C.byref(d), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return self


def episode_groups(model, feet, q, v, start_step, v_des, w_des, gait, sim_dt=0.001):
    """The other groups of logged episodes on the device: q (B, T, 19), v (B, T, 18) device tensors (views of rows [q, v] are used in
    place), start_step (B,), v_des (B, 3), w_des (B,) or None, gait with gait_period and name.  Returns states (B, T, 43) (the state rows
    of bmpc_id_batch_device: [v | q[0:2] - foot_j[0:2] | q[2:]]), vc_goals (B, T, 5) ([phase_percentage(o), v_des[0:2], w_des, gait value],
    simulation.py:176-187, :491-495, the phase from the integer step o = start_step + r) and com (B, T, 3)
    (bmpc_ik_centroidal_state_device).  No kernel of its own."""
    import torch
    from . import _lib, dataset
    from .inverse_kinematics_cpp import as_device_model
    from .robot_id_controller import id_batch_device
    dm = as_device_model(model)
    B, T = q.shape[0], q.shape[1]
    n, dev = B * T, q.device
    f64 = dict(dtype=torch.float64, device=dev)
    in_place = (B > 0 and q.stride(2) == 1 and v.stride(2) == 1 and q.stride(1) == 37 and v.stride(1) == 37 and q.stride(0) == 37 * T and
                v.stride(0) == 37 * T and v.data_ptr() == q.data_ptr() + 19 * 8)
    x = torch.as_strided(q, (n, 37), (37, 1)) if in_place else torch.cat([q.reshape(n, 19), v.reshape(n, 18)], dim=1)
    frames = [dm.model.frame_id(f) for f in feet]
    zeros = torch.zeros((1, 18), **f64)
    states = id_batch_device(dm, frames, 1.0, 0.0, x[:, :19], x[:, 19:], zeros.expand(n, 18), zeros[:, :12].expand(n, 12),
                             want=("state",))["state"].reshape(B, T, 43) if n else torch.zeros((B, T, 43), **f64)
    c9 = torch.empty((n, 9), **f64)
    if n:
        _lib.check(_lib.lib().bmpc_ik_centroidal_state_device(dm.h, C.c_void_p(x.data_ptr()), C.c_void_p(c9.data_ptr()), n,
                                                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    o = torch.as_tensor(start_step, device=dev).to(torch.int64)[:, None] + torch.arange(T, device=dev, dtype=torch.int64)[None, :]
    vc = torch.zeros((B, T, dataset.VC_GOAL_WIDTH), **f64)
    vc[:, :, 0] = torch.remainder(o.to(torch.float64) * sim_dt, gait.gait_period) / gait.gait_period
    vc[:, :, 1:3] = torch.as_tensor(v_des, **f64)[:, None, 0:2]
    if w_des is not None:
        vc[:, :, 3] = torch.as_tensor(w_des, **f64)[:, None]
    vc[:, :, 4] = dataset.GAIT_VALUE.get(getattr(gait, "name", None), 0.0)
    return states, vc, c9[:, 0:3].reshape(B, T, 3).contiguous()
