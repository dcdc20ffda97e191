"""Acyclic motions (jumps, rearing: plans given as time tables) for B robots at once, device resident from the raw states to the
1 kHz rows -- SoloAcyclicGen.optimize (bunmpc_amd/acyclic_gen.py; ISL/examples/mpc/abstract_acyclic_gen.py:298-347) for a batch that
shares one motion table:

    states x = [q, v], times t, motion start times t0
      -> bmpc_acyclic_plan_batch_device    (centroidal state, the tables' rows at every knot time, IK task blocks, per-node regularisation)
      -> bmpc_kinodyn_solve_batch_device   (centroidal ADMM + whole-body IK-DDP)
      -> bmpc_hold_batch_device            (xs_int, us_int, f_int: zero-order hold)

include/ext/bunmpc_acyclic.h declares the first and the last.  torch holds the memory and the stream.  The force maxima of the host
class (25 N) do not enter: the force step projects on the cone, as in the cyclic batch path."""
import ctypes as C

import numpy as np

from . import _lib, _lib_acyclic, problems
from .inverse_kinematics_cpp import as_device_model
from .kinodyn_batch import KinoDynDeviceBatch

EFF_NAMES = ("FL_FOOT", "FR_FOOT", "HL_FOOT", "HR_FOOT")      # abstract_acyclic_gen.py:27

# the plan call's outputs and their shapes per problem, H = T = n_col
_OUTPUTS = {"cnt_plan": lambda H: (H, 4, 4), "dt": lambda H: (H,), "dt_ik": lambda H: (H,), "x_init": lambda H: (9,), "X_nom": lambda H: (9 * H,),
            "X_ter": lambda H: (9,), "bounds": lambda H: (H, 6), "ik_tasks": lambda H: (H + 1, 33), "state_w": lambda H: (H + 1, 36),
            "x_reg": lambda H: (H + 1, 37), "ctrl_w": lambda H: (H, 18)}


def _scalar(v):
    return float(np.asarray(v, dtype=np.float64).reshape(-1)[0])


def host_tables(plan, nq, nv):
    """The time tables of `plan` as the host arrays of a bmpc_acyclic_plan_t ({field: array}, the row counts are their lengths) and
    state_end; ValueError, with the field named, for a list that is empty, too long or of the wrong width.  numpy only.

    State and control regularisation: the lists of one group need not be equally long (the reference's rearing_jump.py has three rows of
    state_wt, two of state_reg and state_scale).  Inside the table, row k of each list holds where state_scale[k]'s window does,
    k < len(state_reg); past state_reg's end every list gives its OWN last row (abstract_acyclic_gen.py:232-254; the control lists the
    same way on len(ctrl_scale) and ctrl_scale's end, :267-289).  The device walks ONE row index per group, so the rows are packed to
    that: the n in-table rows, their windows cut at the end, and one more row [end, +inf) made of each list's last row.  A time below the
    end can only match a row it matched before; a time at or past it only the added row, which is also the last one, the row the device
    takes past the end and for a NaN time."""
    n_col = int(plan.n_col)

    def table(a, shape, name):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != len(shape) or any(n is not None and n != m for n, m in zip(shape, a.shape)):
            raise ValueError("%s: expected shape (%s), got %s" % (name, ", ".join("n" if n is None else "%d" % n for n in shape), a.shape))
        if not 1 <= a.shape[0] <= _lib_acyclic.MAX_PHASES and shape[0] is None:
            raise ValueError("%s: between 1 and %d rows, got %d" % (name, _lib_acyclic.MAX_PHASES, a.shape[0]))
        return a

    def packed(lead, scale, end, lists):
        n = len(lists[lead])
        if n > _lib_acyclic.MAX_PHASES - 1:
            raise ValueError("%s: at most %d rows (one more is added for the times past the end), got %d" % (lead, _lib_acyclic.MAX_PHASES - 1, n))
        for name, a in lists.items():
            if len(a) < n:
                raise ValueError("%s: %d rows, fewer than %s's %d" % (name, len(a), lead, n))
        out = {"tab_" + name: np.concatenate([a[:n], a[-1:]]) for name, a in lists.items()}
        out["tab_" + scale][:n, 2] = np.minimum(out["tab_" + scale][:n, 2], end)
        out["tab_" + scale][n, 1:] = end, np.inf
        return out

    h = dict(dt_arr=table(np.asarray(plan.dt_arr, dtype=np.float64)[:n_col], (n_col,), "dt_arr"),      # (plan_cartwheel.py lists n_col + 1)
             tab_cnt_plan=table(plan.cnt_plan, (None, 4, 6), "cnt_plan"), tab_X_nom=table(plan.X_nom, (None, 11), "X_nom"),
             tab_X_ter=table(plan.X_ter, (9,), "X_ter"), tab_bounds=table(plan.bounds, (None, 8), "bounds"))
    if isinstance(plan.swing_wt, (np.ndarray, list)):      # None or a scalar: no swing tasks (:204)
        h["tab_swing_wt"] = table(plan.swing_wt, (None, 4, 6), "swing_wt")
    state_reg = table(plan.state_reg, (None, nq + nv + 2), "state_reg")
    state_end = float(state_reg[-1, -1])
    h.update(packed("state_reg", "state_scale", state_end, dict(state_reg=state_reg[:, :nq + nv], state_wt=table(plan.state_wt, (None, 2 * nv + 2), "state_wt")[:, :2 * nv],
                                                                state_scale=table(plan.state_scale, (None, 3), "state_scale"))))
    ctrl_scale = table(plan.ctrl_scale, (None, 3), "ctrl_scale")
    h.update(packed("ctrl_scale", "ctrl_scale", float(ctrl_scale[-1, -1]), dict(ctrl_wt=table(plan.ctrl_wt, (None, nv + 2), "ctrl_wt")[:, :nv], ctrl_scale=ctrl_scale)))
    return {k: np.ascontiguousarray(a) for k, a in h.items()}, state_end


class DeviceMotionTable:
    """An ACyclicMotionParams-shaped object (motions/weight_abstract.py; the reference's own motions/acyclic/*.py work as they are)
    uploaded once: every time table as one device tensor, the row counts and scalars on the host."""

    def __init__(self, plan, model, eff_names=EFF_NAMES, device="cuda"):
        import torch
        self.torch, self.device = torch, torch.device(device)
        self.plan = plan
        self.dm = as_device_model(model)
        nq, nv = self.dm.model.nq, self.dm.model.nv
        self.n_col = int(plan.n_col)
        h, self.state_end = host_tables(plan, nq, nv)
        self.host, swing = h, "tab_swing_wt" in h
        self.counts = dict(n_cnt=len(h["tab_cnt_plan"]), n_x=len(h["tab_X_nom"]), n_b=len(h["tab_bounds"]), n_sw=len(h["tab_swing_wt"]) if swing else 0,
                           n_s=len(h["tab_state_scale"]), n_c=len(h["tab_ctrl_scale"]))
        self.cnt_wt, self.cent_wt = _scalar(plan.cnt_wt), (_scalar(plan.cent_wt[0]), _scalar(plan.cent_wt[1]))
        self.foot_frame = [self.dm.model.frame_id(n) for n in eff_names]
        self.dev = {k: torch.from_numpy(a).to(self.device) for k, a in h.items()}
        # rows of the 1 kHz plan: the IK stage's dt is dt_arr itself, so every problem has the same (:331-345)
        self.rows = int(sum(int(v / 0.001) for v in h["dt_arr"]))

    def fill(self, d):
        """the table's fields of a bmpc_acyclic_plan_t"""
        d.n_col, d.model = self.n_col, self.dm.h
        for k, v in self.counts.items():
            setattr(d, k, v)
        for j in range(4):
            d.foot_frame[j] = self.foot_frame[j]
        d.cnt_wt, d.cent_wt[0], d.cent_wt[1], d.state_end = self.cnt_wt, self.cent_wt[0], self.cent_wt[1], self.state_end
        for k, v in self.dev.items():
            setattr(d, k, v.data_ptr())


class DeviceAcyclicPlan:
    """The plan tensors of one batch on the table's device (bmpc_acyclic_plan_batch_device): build() fills them from x (B, 37), t (B,),
    t0 (B,); load_host(arrays) fills the same tensors from host arrays instead (a plan built elsewhere: tests/acyclic_np.py).  What
    batch.DeviceBatch(plan=..., plan_bounds=True) and kinodyn_batch.KinoDynDeviceBatch(plan=..., plan_costs=True) take."""

    def __init__(self, table, B, x=None, t=None, t0=None):
        torch = self.torch = table.torch
        self.table, self.device = table, table.device
        self.B, self.H, self.T = int(B), table.n_col, table.n_col
        f64 = torch.float64
        self.x = torch.zeros((self.B, 37), dtype=f64, device=self.device)
        self.t, self.t0 = torch.zeros(self.B, dtype=f64, device=self.device), torch.zeros(self.B, dtype=f64, device=self.device)
        for name, shape in _OUTPUTS.items():
            setattr(self, name, torch.zeros((self.B,) + shape(self.H), dtype=f64, device=self.device))
        self.status = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self.inp = dict(x_init=self.x_init)      # DeviceBatch(plan=...) reads x_init from here
        d = _lib_acyclic.AcyclicPlan()
        table.fill(d)
        d.B = self.B
        for k in ("x", "t", "t0", "status") + tuple(_OUTPUTS):
            setattr(d, k, getattr(self, k).data_ptr())
        self.desc = d
        if x is not None:
            self.update(x, t, t0)

    def _copy(self, dst, src):
        torch = self.torch
        src = src if isinstance(src, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(src), dtype=dst.dtype)
        if tuple(src.shape) != tuple(dst.shape):
            raise ValueError("expected shape %s, got %s" % (tuple(dst.shape), tuple(src.shape)))
        dst.copy_(src)

    def update(self, x, t, t0):
        """new states, times and motion start times for the same batch size, copied into the tensors the descriptor points at"""
        for dst, src in ((self.x, x), (self.t, t), (self.t0, t0)):
            self._copy(dst, src)
        return self

    def build(self):
        """asynchronous on torch's current stream"""
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib_acyclic.lib().bmpc_acyclic_plan_batch_device(C.byref(self.desc), C.c_void_p(stream)))
        return self

    def load_host(self, arrays):
        """the outputs (and x) from host arrays {name: array}; every output must be given"""
        missing = sorted((set(_OUTPUTS) | {"x"}) - set(arrays))
        if missing:
            raise ValueError("load_host: missing " + ", ".join(missing))
        for name in tuple(_OUTPUTS) + ("x",):
            self._copy(getattr(self, name), np.asarray(arrays[name], dtype=np.float64).reshape(tuple(getattr(self, name).shape)))
        self.status.zero_()
        return self

    def arrays(self):
        """the tensors as host arrays: what load_host takes, and status"""
        self.torch.cuda.synchronize(self.device)
        return {k: getattr(self, k).cpu().numpy() for k in tuple(_OUTPUTS) + ("x", "status")}


def hold_on_device(knots, dt, size, max_rows=None, step=0.001, out=None, rows=None):
    """Zero-order-hold 1 kHz plan of a batch of knot trajectories (bmpc_hold_batch_device): knots (B, n, w), dt (B, >= size) device
    tensors -> (out (B, max_rows, w), rows (B,)); out[b, :rows[b]] = vstack_i tile(knots[b][i], int(dt[b][i] / step)), clipped at
    max_rows (None: the longest problem's, read back from dt).  out, rows: tensors of an earlier call to write into."""
    import torch
    B, n, w = knots.shape
    knots, dt = knots.contiguous(), dt.contiguous()
    if max_rows is None:
        # the kernel's hold_count on the host, in numpy: torch divides a device tensor by a scalar as a multiply by its reciprocal,
        # and (k / 1000) * (1 / 0.001) is k where the correctly rounded (k / 1000) / 0.001 is just below it (k = 43, 51, 59, ...)
        q = dt[:, :size].cpu().numpy() / step
        max_rows = max(int(np.where(q >= 1.0, np.minimum(q, 1073741824.0), 0.0).astype(np.int64).sum(axis=1).max()), 1)
    if out is None:
        out = torch.zeros((B, max_rows, w), dtype=torch.float64, device=knots.device)
        rows = torch.zeros(B, dtype=torch.int32, device=knots.device)
    d = _lib_acyclic.HoldBatch()
    d.B, d.n_knots, d.width, d.size, d.max_rows, d.dt_stride, d.step = B, n, w, size, max_rows, dt.shape[1], step
    d.knots, d.dt, d.out, d.rows = knots.data_ptr(), dt.data_ptr(), out.data_ptr(), rows.data_ptr()
    stream = torch.cuda.current_stream(knots.device).cuda_stream
    _lib.check(_lib_acyclic.lib().bmpc_hold_batch_device(C.byref(d), C.c_void_p(stream)))
    return out, rows


class BatchedAcyclicMpc:
    def __init__(self, model, plan, dyn_iters=50, device="cuda", eff_names=EFF_NAMES, mu=1.0):
        """plan: an ACyclicMotionParams-shaped object, one motion for the whole batch; dyn_iters: kd.optimize(q, v, 50, 1) (:319)"""
        self.model, self.plan, self.dyn_iters, self.device, self.mu = model, plan, dyn_iters, device, mu
        self.table = DeviceMotionTable(plan, model, eff_names, device)
        self.H = self.T = self.table.n_col
        self._kb = self._plan = self._int = None

    def make_solver(self, plan):
        """the KinoDyn batch that solves `plan` (a DeviceAcyclicPlan of this table)"""
        return KinoDynDeviceBatch(self._weights_only_batch(plan.B), self.table.dm, device=self.device, num_iters=self.dyn_iters, plan=plan, plan_costs=True)

    def optimize(self, x, t, t0):
        """x (B, 37), t (B,), t0 (B,) numpy arrays or device tensors -> dict of device tensors: xs_int (B, R, 37), us_int (B, R, 18),
        f_int (B, R, 12), rows (B,) valid rows of each, plus the raw solution (xs, us, X, F) and `plan`.  Everything is a view of
        buffers that the next call with the same batch size reuses: copy what has to outlive it."""
        B = int(x.shape[0])
        if self._kb is not None and self._plan.B == B:
            plan, kb = self._plan.update(x, t, t0).build(), self._kb
        else:
            plan = DeviceAcyclicPlan(self.table, B, x, t, t0).build()
            kb, self._int = self.make_solver(plan), {}
        kb.solve()
        T, H, o = self.T, self.H, kb.off
        xs = kb.ws[:, o["xs"]:o["xs"] + (T + 1) * 37].reshape(B, T + 1, 37)
        us = kb.ws[:, o["us"]:o["us"] + T * 18].reshape(B, T, 18)
        F = kb.dyn.F.reshape(B, H, 12)
        out = {}
        for name, knots in (("xs_int", xs), ("us_int", us), ("f_int", F)):      # dt_arr[T] = 0: the terminal state gets no row (:331-345)
            keep = self._int.get(name, (None, None))
            self._int[name] = hold_on_device(knots, plan.dt_ik, T, max(self.table.rows, 1), out=keep[0], rows=keep[1])
            out[name] = self._int[name][0]
        self._kb, self._plan = kb, plan
        out.update(rows=self._int["xs_int"][1], xs=xs, us=us, X=kb.dyn.X, F=kb.dyn.F, plan=plan, solver=kb)
        return out

    def _weights_only_batch(self, B):
        """the small host-provided part of a WholeBodyBatch: centroidal weights, rho, CoM / momentum tracking weights (everything per
        problem comes from the device plan: placeholders of the right type here, never uploaded)"""
        p, H, T = self.plan, self.H, self.T
        z = lambda *shape: np.broadcast_to(0.0, shape)       # noqa: E731 -- shape-only stand-ins, no memory behind them
        f = lambda a: np.asarray(a, dtype=np.float64)        # noqa: E731
        dyn = problems.Batch("acyclic", B, H, 4, self.table.dm.model.total_mass, float(p.rho), z(B, H, 4, 4), z(B, H), z(B, 9), z(B, 9 * H), z(B, 9),
                             np.tile(f(p.W_X), H)[None], f(p.W_X_ter)[None].copy(), np.tile(f(p.W_F), H)[None], z(B, H, 6), None, None, self.mu, {})
        return problems.WholeBodyBatch(dyn, z(B, 37), T, z(B, T + 1, 33), z(B, T + 1, 36), z(B, T, 18), z(B, T + 1, 37), self.table.cent_wt[0],
                                       self.table.cent_wt[1], ())
