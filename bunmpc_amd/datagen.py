"""One device-resident pass of the reference's data generation, from nominal states to training rows:

    nominal (q, v), t0, desired velocity (and, with step(..., w_des=...), desired yaw rate: the turning commands of the reference's
    sampler, utils.get_des_velocities)
      -> contact flags of the current knot                      (bmpc_wb_plan_batch_device, plan of the nominal state)
      -> contact-conditioned perturbation + foot-height rejection    (bmpc_perturb_batch_device; data_collection.py:188-262)
      -> plan inputs of the perturbed state, KinoDynMP.optimize, 1 kHz plan   (BatchedMpc; abstract_cyclic_gen.py:629-698)
      -> inverse-dynamics controller, pd_target action, policy state     (bmpc_id_batch_device; simulation.py:484-528)

What the reference has between the last two steps -- a PyBullet rollout that feeds the measured state back every
millisecond -- is out of scope (simulator), so the rows produced here are the expert's labels ON its own plan:
row r of problem b is (state, action) of the plan's r-th millisecond with the measured state equal to the planned one,
row 0 being the perturbed state itself.

The contact-conditioned goals (`cc_goals`) are an opt-in (goal_horizon >= 1): the planner-derived goals a contact-conditioned policy
is conditioned on where the reference deploys it (simulation.py:999-1006: Raibert schedule of the perturbed state, estimated CoM,
construct_cc_goal), built on the device by bmpc_cc_goal_wb_batch_device (cc_goal_batch.py) -- for the expert's labels on its own
plan the consistent goal.  The goals the reference's data collection builds from contacts MEASURED in the simulator
(simulation.py:563-568) stay out of scope."""
import numpy as np

from . import dataset, problems
from .mpc_batch import BatchedMpc
from .perturbation import PerturbationSampler
from .robot_id_controller import id_batch_device


class PlanLabelGenerator:
    def __init__(self, model, gait=problems.TROT, ik=problems.TROT_IK, wb=problems.SOLO12_WB, kp=3.0, kd=0.05,
                 mu=(0.0, 0.0, 0.0, 0.0), sigma=(0.05, 0.1, 0.2, 0.2), planning_time=0.05, dyn_iters=10, draws_per_call=4,
                 device="cuda:0", goal_horizon=0, episode_length=3000, com="estimated"):
        """goal_horizon: 0 (default) builds no cc_goals -- step() launches and returns what it always did; >= 1: step() also returns
        cc_goals for an episode of episode_length steps that starts at t = 0.  com: "estimated" (round(com(q0), 3) + i sim_dt v_des, the
        reference's deployment) or "plan" (the CoM of the planned states xs_int, bmpc_ik_centroidal_state_device)."""
        if goal_horizon < 0 or com not in ("estimated", "plan"):
            raise ValueError("goal_horizon must be >= 0 and com 'estimated' or 'plan'")
        self.goal_horizon, self.episode_length, self.goal_com, self._goals = int(goal_horizon), int(episode_length), com, None
        self.mpc = BatchedMpc(model, gait, ik, wb, planning_time=planning_time, dyn_iters=dyn_iters, device=device)
        self.sampler = PerturbationSampler(self.mpc.dm, wb.feet, mu, sigma, draws_per_call=draws_per_call, device=device)
        self.foot_frames = [model.frame_id(n) for n in wb.feet]
        self.kp, self.kd, self.gait, self.wb = kp, kd, gait, wb
        self.rows_per_plan = int(round(planning_time / 0.001))
        self._nominal = None

    def step(self, q_nom, v_nom, t0, v_des_body, generator=None, perturb=True, episode_length=None, w_des=None):
        """q_nom (B,19), v_nom (B,18), t0 (B,), v_des_body (B,3): device tensors.  w_des (B,): desired yaw rates, a device tensor --
        they reach the nominal plan, the MPC call and the cc_goals, and fill vc_goals[:, :, 3] (the row is [phase, v_x, v_y, w_des, gait],
        simulation.py:494); None: w_des = 0 everywhere, through the calls that take no command.  Returns device tensors
        states (B,R,43), actions (B,R,12), vc_goals (B,R,5), and q0 / v0 (the perturbed initial states), `rejected`
        (indices whose draws were all refused: those keep their nominal state).  With goal_horizon >= 1 also cc_goals
        (B,R,12 goal_horizon), goal_rows (B,) int32 -- rows of cc_goals[b] that hold goals, zeros behind them -- and goal_status (B,)
        int32, the BMPC_CC_* bits of include/bunmpc_goals.h (0: every row there); episode_length: the episode's length in steps for
        these goals (default: the constructor's)."""
        import torch
        from .plan_batch import DeviceWbPlan
        m = self.mpc
        B = q_nom.shape[0]
        rejected = torch.empty(0, dtype=torch.long, device=q_nom.device)
        if perturb:
            x = torch.cat([q_nom, v_nom], dim=1)
            x[:, 0:2] = 0.0
            if self._nominal is not None and self._nominal.B == B:
                nominal = self._nominal.update(x, t0, v_des_body, w_des=w_des).build()
            else:
                nominal = self._nominal = DeviceWbPlan(m.dm, m.gait, m.offsets_xy, m.wb.feet, m.ik, x, t0, v_des_body, m.H, m.T,
                                                       device=m.device, w_des=w_des, yaw_inertia=m.yaw_inertia).build()
            q0, v0, rejected = self.sampler.sample(q_nom, v_nom, nominal.cnt_plan[:, 0, :, 0], generator=generator)
        else:
            q0, v0 = q_nom, v_nom
        sol = m.optimize(torch.cat([q0, v0], dim=1), t0, v_des_body, w_des=w_des)
        R = min(self.rows_per_plan, int(sol["rows"].min()))
        xs = sol["xs_int"][:, :R].reshape(B * R, 37)
        us = sol["us_int"][:, :R].reshape(B * R, 18)
        f = sol["f_int"][:, :R].reshape(B * R, 12)
        out = id_batch_device(m.dm, self.foot_frames, self.kp, self.kd, xs[:, :19], xs[:, 19:], us, f, want=("action", "state"))
        t = (t0[:, None] + 0.001 * torch.arange(R, device=t0.device, dtype=torch.float64)[None, :])
        vc = torch.zeros((B, R, dataset.VC_GOAL_WIDTH), dtype=torch.float64, device=t0.device)
        vc[:, :, 0] = torch.remainder(t, self.gait.gait_period) / self.gait.gait_period
        vc[:, :, 1:3] = v_des_body[:, None, 0:2]
        if w_des is not None:
            vc[:, :, 3] = w_des[:, None]
        vc[:, :, 4] = dataset.GAIT_VALUE.get(self.gait.name, 0.0)
        res = dict(states=out["state"].reshape(B, R, 43), actions=out["action"].reshape(B, R, 12), vc_goals=vc, q0=q0, v0=v0,
                   rejected=rejected, solution=sol)
        if self.goal_horizon:
            res.update(self._cc_goals(torch.cat([q0, v0], dim=1), t0, v_des_body, xs, R, int(episode_length or self.episode_length), w_des))
        return res

    def _cc_goals(self, x0, t0, v_des, xs, R, episode_length, w_des=None):
        """planner-derived goals of the perturbed states: row r is step int(t0 / 0.001) + r, the step of states[:, r]"""
        import ctypes as C
        import torch
        from . import _lib
        from .cc_goal_batch import DeviceWbCcGoals
        m, B = self.mpc, x0.shape[0]
        if w_des is None:
            w_des = torch.zeros(B, dtype=torch.float64, device=x0.device)      # no command: w_des = 0, as in vc_goals
        g = self._goals
        if g is not None and g.B == B and g.episode_length == episode_length:
            g.update(x0, t0, v_des, w_des)
        else:
            g = self._goals = DeviceWbCcGoals(m.dm, self.gait, self.wb.feet, self.wb.hips, episode_length, x0, t0, v_des, w_des,
                                              goal_horizon=self.goal_horizon, max_rows=self.rows_per_plan, com_rows=self.goal_com == "plan",
                                              device=m.device)
        if self.goal_com == "plan":
            c9 = torch.empty((B * R, 9), dtype=torch.float64, device=x0.device)
            stream = torch.cuda.current_stream(x0.device).cuda_stream
            _lib.check(_lib.lib().bmpc_ik_centroidal_state_device(m.dm.h, C.c_void_p(xs.contiguous().data_ptr()), C.c_void_p(c9.data_ptr()), B * R,
                                                                  C.c_void_p(stream)))
            g.com_rows.zero_()
            g.com_rows[:, :R] = c9[:, 0:3].reshape(B, R, 3)
        g.build()
        rows = torch.clamp(g.rows, max=R)
        return dict(cc_goals=g.goals[:, :R].clone(), goal_rows=rows, goal_status=g.status.clone())
