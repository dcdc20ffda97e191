"""Contact-conditioned goals built on the GPU (bmpc_cc_goal_batch_device / bmpc_cc_goal_wb_batch_device in include/bunmpc_goals.h):
the Raibert plan over the episode, its switches, the per-foot schedule and the goal rows of B problems, left in HBM.  Device
counterpart of contact_planner.ContactPlanner.get_contact_schedule + goals.get_estimated_com + goals.construct_cc_goal as the
reference chains them where it deploys a contact-conditioned policy (simulation.py:999-1006): the goal's episode length is
episode_length + 1 and its first row is step int(t0 / sim_dt)."""
import ctypes as C

import numpy as np

from . import _lib

# the bits of `status` (include/bunmpc_goals.h)
FEW_SWITCHES, START_AFTER_END, PAST_SCHEDULE, EVENTS_OVERFLOW = (
    _lib._ABI.defines["BMPC_CC_" + n] for n in ("FEW_SWITCHES", "START_AFTER_END", "PAST_SCHEDULE", "EVENTS_OVERFLOW"))


def gait_struct(gait):
    g = _lib.CcGait()
    g.gait_period, g.gait_dt, g.gait_horizon = gait.gait_period, gait.gait_dt, gait.gait_horizon
    for j in range(4):
        g.stance_percent[j], g.phase_offset[j] = gait.stance_percent[j], gait.phase_offset[j]
    return g


def plan_knots(episode_length, gait, sim_dt=0.001):
    """H_cp of contact_planner.py:130, through the C-ABI (no GPU)"""
    return _lib.lib().bmpc_cc_goal_plan_knots(int(episode_length), float(sim_dt), float(gait.gait_horizon), float(gait.gait_period), float(gait.gait_dt))


def default_max_events(gait, episode_length, sim_dt=0.001):
    """room for every switch of a plan: each foot touches down once per gait period, plus one per foot for the ends"""
    H = plan_knots(episode_length, gait, sim_dt)
    return max(2, 4 * (int(H * gait.gait_dt / gait.gait_period) + 2))


class _GoalTensors:
    def _outputs(self, d, B, H, goal_horizon, max_rows, max_events, want_plan, com_rows):
        torch, f64 = self.torch, self.torch.float64

        def z(*shape, dtype=f64):
            return torch.empty(shape, dtype=dtype, device=self.device)

        self.goals, self.rows, self.status = z(B, max_rows, 12 * goal_horizon), z(B, dtype=torch.int32), z(B, dtype=torch.int32)
        self.schedule, self.counts = z(B, 4, max_events, 4), z(B, 4, dtype=torch.int32)
        self.cnt_plan, self.swing_time = (z(B, H, 4, 4), z(B, H, 4)) if want_plan else (None, None)
        self.com_rows = z(B, max_rows, 3) if com_rows else None
        for k in ("goals", "rows", "status", "schedule", "counts", "cnt_plan", "swing_time", "com_rows"):
            v = getattr(self, k)
            setattr(d, k, None if v is None else v.data_ptr())

    def _sizes(self, d, gait, B, episode_length, goal_horizon, max_rows, max_events, sim_dt):
        d.B, d.n_eff, d.episode_length, d.goal_horizon = B, len(gait.stance_percent), episode_length, goal_horizon
        d.max_rows, d.max_events, d.sim_dt, d.gait = max_rows, max_events, sim_dt, gait_struct(gait)
        d.n_knots = self.H = plan_knots(episode_length, gait, sim_dt)
        self.episode_length = episode_length
        if self.H < 1:
            raise ValueError("episode_length %d gives a plan of %d knots: nothing to plan" % (episode_length, self.H))

    def _up(self, a, dtype=None):
        torch = self.torch
        dtype = dtype or torch.float64
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=self.device).contiguous()

    def _set(self, pairs):
        torch = self.torch
        for dst, src in pairs:
            dst.copy_(src if isinstance(src, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(src), dtype=torch.float64))
        return self


class DeviceCcGoals(_GoalTensors):
    """From arrays (numpy or torch): t0 (B,), com (B,3) and feet0 (B,4,3) unrounded, hip_off (B,4,2) = (R_yaw offsets[j])[0:2],
    v_des (B,3) as the planner takes it, w_des (B,).  com_rows=True: the goals use the CoM rows the caller writes to
    `com_rows` (B, max_rows, 3) before build(); False: the estimated CoM.  Results are device tensors: goals (B, max_rows,
    12 goal_horizon) with zeros from row rows[b] on, rows, status (the BMPC_CC_* bits), schedule (B, 4, max_events, 4), counts and,
    with want_plan, cnt_plan (B, H_cp, 4, 4) and swing_time."""

    def __init__(self, gait, episode_length, t0, com, feet0, hip_off, v_des, w_des, goal_horizon=1, max_rows=None, max_events=None,
                 com_rows=False, want_plan=False, sim_dt=0.001, device="cuda"):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceCcGoals needs a GPU")
        self.torch, self.device = torch, torch.device(device)
        B = int(np.shape(t0)[0])
        max_rows = episode_length + 1 if max_rows is None else max_rows
        max_events = default_max_events(gait, episode_length, sim_dt) if max_events is None else max_events
        d = _lib.CcGoalBatch()
        self._sizes(d, gait, B, episode_length, goal_horizon, max_rows, max_events, sim_dt)
        self.B = B
        self.inp = dict(t0=self._up(t0), com=self._up(com), feet0=self._up(feet0), hip_off=self._up(hip_off), v_des=self._up(v_des), w_des=self._up(w_des))
        for k, v in self.inp.items():
            setattr(d, k, v.data_ptr())
        self._outputs(d, B, self.H, goal_horizon, max_rows, max_events, want_plan, com_rows)
        self.desc = d

    def update(self, **arrays):
        """new inputs for the same batch size, copied into the tensors the descriptor points at"""
        return self._set((self.inp[k], v) for k, v in arrays.items())

    def build(self):
        """asynchronous on torch's current stream"""
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib.lib().bmpc_cc_goal_batch_device(C.byref(self.desc), C.c_void_p(stream)))
        return self


class DeviceWbCcGoals(_GoalTensors):
    """From whole-body states x (B,37) = [q, v] of the robot of dev_model: the kinematics, the hip offsets of the current q and the
    rest as DeviceCcGoals.  feet / hips: frame names (eff_names, hip_names).  Intermediates the front end writes: com (B,3),
    feet0 (B,4,3), hips (B,4,3), hip_off (B,4,2)."""

    def __init__(self, dev_model, gait, feet, hips, episode_length, x, t0, v_des, w_des, goal_horizon=1, max_rows=None, max_events=None,
                 com_rows=False, want_plan=False, sim_dt=0.001, device="cuda"):
        import torch
        self.torch, self.device = torch, torch.device(device)
        B = int(x.shape[0])
        max_rows = episode_length + 1 if max_rows is None else max_rows
        max_events = default_max_events(gait, episode_length, sim_dt) if max_events is None else max_events
        d = _lib.CcGoalWbBatch()
        self._sizes(d.g, gait, B, episode_length, goal_horizon, max_rows, max_events, sim_dt)
        self.B, self.dev_model = B, dev_model
        d.model = dev_model.h
        for j in range(4):
            d.foot_frame[j], d.hip_frame[j] = dev_model.model.frame_id(feet[j]), dev_model.model.frame_id(hips[j])
        self.x, self.t0, self.v_des, self.w_des = self._up(x), self._up(t0), self._up(v_des), self._up(w_des)
        f64 = torch.float64
        self.com, self.feet0 = torch.empty((B, 3), dtype=f64, device=self.device), torch.empty((B, 4, 3), dtype=f64, device=self.device)
        self.hips, self.hip_off = torch.empty((B, 4, 3), dtype=f64, device=self.device), torch.empty((B, 4, 2), dtype=f64, device=self.device)
        d.x = self.x.data_ptr()
        for k in ("com", "feet0", "hips", "hip_off"):
            setattr(d, k, getattr(self, k).data_ptr())
        for k in ("t0", "v_des", "w_des"):
            setattr(d.g, k, getattr(self, k).data_ptr())
        self._outputs(d.g, B, self.H, goal_horizon, max_rows, max_events, want_plan, com_rows)
        self.desc = d

    def update(self, x, t0, v_des, w_des=None):
        return self._set([(self.x, x), (self.t0, t0), (self.v_des, v_des)] + ([] if w_des is None else [(self.w_des, w_des)]))

    def build(self):
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib.lib().bmpc_cc_goal_wb_batch_device(C.byref(self.desc), C.c_void_p(stream)))
        return self
