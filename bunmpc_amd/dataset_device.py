"""The trainers' data set kept on the device (include/ext/bunmpc_dataset.h): the ring buffer, input statistics and batch view of the
reference's `Database` (`ISL/examples/iterative_algorithm/database.py`) for rows that are device tensors already -- what
`PlanLabelGenerator.step()` returns -- so that nothing crosses to the host between the generator and a trainer:

    out = generator.step(...)
    db.append_step(out)                  # kernels on torch's current stream; no synchronisation, no copy to the host
    db.calc_input_mean_std()             # per-column mean and std of states and cc_goals over rows [0, length)
    x, y = db.batch(index)               # [state | goal], action of the rows `index`, normalised as __getitem__ does

torch holds the memory and the stream.  `bunmpc_amd/dataset.py::Database` stays the host class and the way to disk: `to_host()`,
`from_host()`, `arrays()` and `save()` go through it."""
import ctypes as C

import numpy as np

from . import _lib, _lib_dataset, dataset


class DeviceDatabase:
    def __init__(self, limit, n_eff=4, goal_horizon=1, device="cuda", norm_input=True, goal_type="cc", max_problems=1 << 18):
        """goal_horizon = 0: a data set without the cc_goals group.  max_problems: the largest number of problems (rows, for appends
        given as (n, w)) one append may bring; it sizes the device scratch (12 bytes each)."""
        import torch
        self.torch, self.device = torch, torch.device(device)
        self.limit, self.n_eff, self.goal_horizon = int(limit), int(n_eff), int(goal_horizon)
        self.w_cc = 3 * self.n_eff * self.goal_horizon
        self.norm_input = True
        self.set_normalize_input(norm_input)
        self.goal_type = None
        self.set_goal_type(goal_type)
        d = _lib_dataset.Dataset()
        d.limit, d.max_problems = self.limit, int(max_problems)
        d.w_states, d.w_vc, d.w_cc, d.w_actions = _lib_dataset.STATE_WIDTH, _lib_dataset.VC_WIDTH, self.w_cc, _lib_dataset.ACTION_WIDTH
        nbytes = _lib_dataset.lib().bmpc_dataset_scratch_bytes(d.limit, d.w_cc, d.max_problems)
        if nbytes < 0:
            raise ValueError("limit must be in [1, 2^31), 3 n_eff goal_horizon a multiple of 3 in [0, %d], max_problems in [1, %d]; got %d, %d, %d"
                             % (_lib_dataset.MAX_CC_WIDTH, _lib_dataset.MAX_PROBLEMS, self.limit, self.w_cc, d.max_problems))
        f64 = dict(dtype=torch.float64, device=self.device)
        self.states = torch.zeros((self.limit, d.w_states), **f64)
        self.vc_goals = torch.zeros((self.limit, d.w_vc), **f64)
        self.cc_goals = torch.zeros((self.limit, d.w_cc), **f64)
        self.actions = torch.zeros((self.limit, d.w_actions), **f64)
        self.header = torch.zeros(_lib_dataset.HEADER_LONGS, dtype=torch.int64, device=self.device)
        self._scratch = torch.zeros((nbytes + 15) // 16 * 2, dtype=torch.int64, device=self.device)
        d.states, d.vc_goals, d.actions = self.states.data_ptr(), self.vc_goals.data_ptr(), self.actions.data_ptr()
        d.cc_goals = self.cc_goals.data_ptr() if d.w_cc else None
        d.header, d.scratch, d.scratch_bytes = self.header.data_ptr(), self._scratch.data_ptr(), nbytes
        self.desc = d
        self.states_mean = self.states_std = self.cc_goals_mean = self.cc_goals_std = None
        self.vc_goals_mean, self.vc_goals_std = 0.0, 1.0          # database.py:201-202

    # ---- the reference's switches (database.py:85-102) -------------------------------------------------------------------------------
    def set_normalize_input(self, value):
        self.norm_input = bool(value)

    def set_goal_type(self, value):
        if value not in ("vc", "cc"):
            raise ValueError("Goal type can only be vc or cc")
        self.goal_type = value

    # ---- the ring ----------------------------------------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def append(self, states, actions, vc_goals=None, cc_goals=None, rows=None, keep=None, drop_nonfinite=False):
        """states (n, 43) or (B, R, 43) device tensors, the other groups alike; rows (B,) int32: leading rows of problem b that go in
        (clipped to [0, R]); keep (B,): 0 drops problem b; drop_nonfinite: a problem whose kept rows hold a NaN or an infinity in a given
        group brings no row.  (n, w) is n problems of one row.  Kernels on torch's current stream; does not synchronise."""
        torch = self.torch
        if vc_goals is None and cc_goals is None:
            raise ValueError("both vc_goals and cc_goals cant be empty!")
        if states.dim() not in (2, 3):
            raise ValueError("states: expected (n, 43) or (B, R, 43), got %s" % (tuple(states.shape),))
        B, R = (states.shape[0], 1) if states.dim() == 2 else (states.shape[0], states.shape[1])
        r = _lib_dataset.DatasetRows()
        empty = B == 0 or R == 0        # the call still runs: the header's count of appended rows becomes 0
        r.B, r.R, r.drop_nonfinite = (0, 1, 0) if empty else (B, R, int(bool(drop_nonfinite)))
        hold = []
        widths = dict(states=self.desc.w_states, actions=self.desc.w_actions, vc_goals=self.desc.w_vc, cc_goals=self.desc.w_cc)
        for name, t in (("states", states), ("actions", actions), ("vc_goals", vc_goals), ("cc_goals", cc_goals)):
            w = widths[name]
            if t is not None:
                if t.dtype != torch.float64 or t.device != self.states.device:
                    raise ValueError("%s: a float64 tensor on %s is expected, got %s on %s" % (name, self.states.device, t.dtype, t.device))
                if tuple(t.shape[:-1]) != tuple(states.shape[:-1]):
                    raise ValueError("%s: leading shape %s differs from that of states %s" % (name, tuple(t.shape[:-1]), tuple(states.shape[:-1])))
                w = t.shape[-1]
                t = t.contiguous()
                hold.append(t)
                setattr(r, name, self.states.data_ptr() if empty else t.data_ptr())      # (an empty tensor has no address; nothing is read)
            setattr(r, "w_" + ("vc" if name == "vc_goals" else "cc" if name == "cc_goals" else name), w)
        for name, t in (("rows", rows), ("keep", keep)):
            if t is not None:
                t = torch.as_tensor(t, device=self.device).to(torch.int32).contiguous()
                if tuple(t.shape) != (B,):
                    raise ValueError("%s: expected shape (%d,), got %s" % (name, B, tuple(t.shape)))
                hold.append(t)
                setattr(r, name, None if empty else t.data_ptr())
        # (`hold` keeps the contiguous copies alive until the kernels are enqueued; freed after that, their memory is reused in stream order)
        _lib.check(_lib_dataset.lib().bmpc_dataset_append_device(C.byref(self.desc), C.byref(r), self._stream()))
        return self

    def append_step(self, out, drop_rejected=False, drop_nonfinite=True):
        """the dict PlanLabelGenerator.step() returns: every problem's rows with vc_goals; with cc_goals in it, rows = goal_rows and a
        problem with a nonzero goal_status brings no row; drop_rejected: nor do the problems of out["rejected"] (whose draws were all
        refused: they kept their nominal state).  Does not synchronise."""
        torch = self.torch
        B = out["states"].shape[0]
        rows = keep = cc = None
        if "cc_goals" in out and self.w_cc:
            cc, rows = out["cc_goals"], out["goal_rows"]
            keep = (out["goal_status"] == 0).to(torch.int32)
        if drop_rejected and out["rejected"].numel():
            keep = torch.ones(B, dtype=torch.int32, device=self.device) if keep is None else keep
            keep = keep.index_fill(0, out["rejected"].to(torch.long), 0)
        return self.append(out["states"], out["actions"], vc_goals=out["vc_goals"], cc_goals=cc, rows=rows, keep=keep, drop_nonfinite=drop_nonfinite)

    def append_episodes(self, states, actions, vc_goals, log):
        """logged episodes: states (B, T, 43), actions (B, T, 12), vc_goals (B, T, 5) and a built contact_log.DeviceContactLog -- the
        leading log.rows[b] rows of every group with the measured goals, nothing of an episode with a nonzero status (the reference
        returns nothing for those).  Does not synchronise."""
        R = log.goals.shape[1]      # max_rows <= T
        return self.append(states[:, :R], actions[:, :R], vc_goals=vc_goals[:, :R], cc_goals=log.goals, rows=log.rows,
                           keep=(log.status == 0).to(self.torch.int32))

    def _header(self):
        h = self.header.cpu()
        return int(h[0]), int(h[1]), int(h[2])

    @property
    def start(self):
        """reads the device header: synchronises with the stream"""
        return self._header()[0]

    @property
    def length(self):
        """reads the device header: synchronises with the stream"""
        return self._header()[1]

    @property
    def appended(self):
        """rows the last append brought, before the ring dropped any; reads the device header: synchronises with the stream"""
        return self._header()[2]

    def __len__(self):
        """reads the device header: synchronises with the stream"""
        return self.length

    # ---- statistics and batches ---------------------------------------------------------------------------------------------------------
    def calc_input_mean_std(self):
        """states_mean, states_std (43,), cc_goals_mean, cc_goals_std (w_cc,) as device tensors: np.mean / np.std(axis=0) over buffer
        rows [0, length) (database.py:187-213); the vc statistics are the constants 0.0 and 1.0.  Does not synchronise."""
        torch = self.torch
        f64 = dict(dtype=torch.float64, device=self.device)
        sm, ss = torch.empty(self.desc.w_states, **f64), torch.empty(self.desc.w_states, **f64)
        cm, cs = torch.empty(self.w_cc, **f64), torch.empty(self.w_cc, **f64)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None      # noqa: E731
        _lib.check(_lib_dataset.lib().bmpc_dataset_moments_device(C.byref(self.desc), ptr(sm), ptr(ss), ptr(cm), ptr(cs), self._stream()))
        self.states_mean, self.states_std = sm, ss
        if self.w_cc:
            self.cc_goals_mean, self.cc_goals_std = cm, cs
        return self

    def get_database_mean_std(self):
        """[states_mean, states_std, goal_mean, goal_std] of the current goal type, None without norm_input (database.py:215-231)"""
        if not self.norm_input:
            return None
        if self.goal_type == "vc":
            return [self.states_mean, self.states_std, self.vc_goals_mean, self.vc_goals_std]
        return [self.states_mean, self.states_std, self.cc_goals_mean, self.cc_goals_std]

    def batch(self, index):
        """(x, y) device tensors for the buffer rows `index` (int64, any shape (n,)): x[i] = [state | goal] (normalised with the
        statistics of the last calc_input_mean_std() when norm_input is set), y[i] = action -- the rows DataLoader would collate from
        __getitem__.  An index outside [0, length) gives a row of NaN.  Does not synchronise."""
        torch = self.torch
        if self.goal_type == "cc" and not self.w_cc:
            raise ValueError("goal type cc on a data set without cc_goals")
        index = torch.as_tensor(index, device=self.device).to(torch.int64).contiguous().reshape(-1)
        n = index.shape[0]
        wg = self.w_cc if self.goal_type == "cc" else self.desc.w_vc
        x = torch.empty((n, self.desc.w_states + wg), dtype=torch.float64, device=self.device)
        y = torch.empty((n, self.desc.w_actions), dtype=torch.float64, device=self.device)
        q = _lib_dataset.DatasetBatch()
        q.n, q.goal_type, q.normalise = n, _lib_dataset.GOAL[self.goal_type], int(self.norm_input)
        q.index, q.x, q.y = index.data_ptr(), x.data_ptr(), y.data_ptr()
        if self.norm_input:
            if self.states_mean is None or (self.goal_type == "cc" and self.cc_goals_mean is None):
                raise ValueError("batch: norm_input is set and calc_input_mean_std() has not run")
            q.states_mean, q.states_std = self.states_mean.data_ptr(), self.states_std.data_ptr()
            if self.goal_type == "cc":
                q.goal_mean, q.goal_std = self.cc_goals_mean.data_ptr(), self.cc_goals_std.data_ptr()
        if n == 0:      # (empty tensors have no address to pass)
            return x, y
        _lib.check(_lib_dataset.lib().bmpc_dataset_batch_device(C.byref(self.desc), C.byref(q), self._stream()))
        return x, y

    # ---- to the host class and back -----------------------------------------------------------------------------------------------------
    def to_host(self):
        """a dataset.Database with the same buffers, start and length (synchronises)"""
        db = dataset.Database(self.limit, n_eff=self.n_eff, goal_horizon=self.goal_horizon)
        db.start, db.length, _ = self._header()
        for k in ("states", "vc_goals", "cc_goals", "actions"):
            setattr(db, k, getattr(self, k).cpu().numpy())
        return db

    @classmethod
    def from_host(cls, db, device="cuda", n_eff=4, **kw):
        """a DeviceDatabase holding the buffers, start and length of a dataset.Database"""
        import torch
        w_cc = db.cc_goals.shape[1]
        if w_cc % (3 * n_eff):
            raise ValueError("cc_goals of width %d are not 3 n_eff goal_horizon wide with n_eff = %d" % (w_cc, n_eff))
        out = cls(db.limit, n_eff=n_eff, goal_horizon=w_cc // (3 * n_eff), device=device, **kw)
        for k in ("states", "vc_goals", "cc_goals", "actions"):
            getattr(out, k).copy_(torch.from_numpy(np.ascontiguousarray(getattr(db, k), dtype=np.float64)))
        out.header.copy_(torch.tensor([db.start, db.length, 0, 0], dtype=torch.int64))
        return out

    def arrays(self):
        return self.to_host().arrays()

    def save(self, directory, iteration, config=None):
        """the file dataset.Database.save writes"""
        return self.to_host().save(directory, iteration, config=config)
