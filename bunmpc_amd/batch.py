"""Batched BiConvex MPC solves on one MI355X: B independent `BiconvexMP.optimize` calls in
one kernel launch (bmpc_biconvex_solve_batch_device / _host in include/bunmpc.h).

`DeviceBatch` keeps a `problems.Batch` resident in HBM as torch tensors (torch is used for
device memory and streams only) and launches on torch's current stream, so
`torch.cuda.Event`s bracket the kernel correctly.  `solve_host` is the numpy-in /
numpy-out path that needs no torch.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import L0_F, L0_X, NSTATS


def _solver_fields(desc, batch, num_iters, maxit, tol, exit_tol, beta, mu):
    mu = batch.mu if mu is None else mu
    desc.B, desc.n_col, desc.n_eff = batch.B, batch.H, batch.E
    desc.num_iters, desc.maxit = num_iters, maxit
    desc.m, desc.rho, desc.mu, desc.beta, desc.tol, desc.exit_tol = batch.m, batch.rho, mu, beta, tol, exit_tol


def _stride(a):
    """batch stride in doubles of a (1 or B, ...) array: 0 when shared"""
    return 0 if a.shape[0] == 1 else int(np.prod(a.shape[1:]))


_COMBINED = "Qx_off / Qf_off (costs between neighbouring knots) cannot be combined with Qx_blk / Qf_blk (per-knot blocks)"


def _cost_ext(kind, B, H, E, x, f, put):
    """bmpc_block_cost_t (kind "blk") of Qx_blk (1 or B, H + 1, 9, 9) / Qf_blk (1 or B, H, 3E, 3E), or bmpc_band_cost_t (kind "off") of
    Qx_off (1 or B, H, 9) / Qf_off (1 or B, H - 1, 3E); either array None.  put(array) -> its address.  None without an array."""
    shapes = {"blk": ((H + 1, 9, 9), (H, 3 * E, 3 * E)), "off": ((H, 9), (H - 1, 3 * E))}[kind]
    c = _lib.BlockCost() if kind == "blk" else _lib.BandCost()
    for name, a, shape in (("Qx_" + kind, x, shapes[0]), ("Qf_" + kind, f, shapes[1])):
        if a is None:
            continue
        if a.shape[1:] != shape or a.shape[0] not in (1, B):
            raise ValueError("%s: expected shape (1 or %d, %s), got %s" % (name, B, ", ".join("%d" % n for n in shape), tuple(a.shape)))
        if a.size:      # (band costs at H = 1: no pair of force knots)
            setattr(c, name, put(a))
            setattr(c, "s" + name, _stride(a))
    return c if getattr(c, "Qx_" + kind) or getattr(c, "Qf_" + kind) else None


PROJECTIONS = {"reference": 0, "euclidean": 1}


def _cone_ext(cone, B, H, E, put):
    """bmpc_cone_t of cone = dict(projection="reference" | "euclidean", mu=None | scalar | array (1 or B, H, E), normals=None | array (1 or B,
    H, E, 3)); put(array) -> its address after whatever copy the caller needs (its result is kept by the caller).  None without a dict.
    With normals: (bmpc_cone_t, bmpc_contact_frame_t)."""
    if cone is None:
        return None
    unknown = set(cone) - {"projection", "mu", "normals"}
    if unknown or cone.get("projection", "reference") not in PROJECTIONS:
        raise ValueError("cone: expected dict(projection=\"reference\" | \"euclidean\", mu=None | array, normals=None | array), got %r" % (cone,))
    c = _lib.Cone(projection=PROJECTIONS[cone.get("projection", "reference")])
    mu = cone.get("mu")
    if mu is not None:
        if np.ndim(mu) == 0:      # one coefficient for every problem, knot and foot
            mu = np.full((1, H, E), float(mu))
        if np.shape(mu)[1:] != (H, E) or np.shape(mu)[0] not in (1, B):
            raise ValueError("cone mu: expected shape (1 or %d, %d, %d), got %s" % (B, H, E, np.shape(mu)))
        c.mu = put(mu)
        c.smu = 0 if np.shape(mu)[0] == 1 else H * E
    normals = cone.get("normals")
    if normals is not None:
        if cone.get("projection", "reference") != "euclidean":
            raise ValueError("cone normals need projection=\"euclidean\": the reference's \"SoC\" step is about world z")
        shape = tuple(normals.shape) if hasattr(normals, "data_ptr") else np.shape(normals)      # (a torch tensor, possibly on a GPU)
        if len(shape) != 4 or shape[1:] != (H, E, 3) or shape[0] not in (1, B):
            raise ValueError("cone normals: expected shape (1 or %d, %d, %d, 3), got %s" % (B, H, E, shape))
        fr = _lib.ContactFrame(normals=put(normals), snormals=0 if shape[0] == 1 else 3 * H * E)
        return c, fr
    return c


def _launch(desc, blocks, band, stream=None, cone=None):
    """the solve call of the batch's cost shape: on `stream` with device arrays, or (None) the host call"""
    lib, where = _lib.lib(), "host" if stream is None else "device"
    tail = () if stream is None else (C.c_void_p(stream),)
    if cone is not None:
        if blocks is not None or band is not None:
            raise ValueError("cone= cannot be combined with Qx_blk / Qf_blk or Qx_off / Qf_off: the cone kernels hold diagonal costs only")
        if isinstance(cone, tuple):      # (with contact normals)
            return _lib.check(getattr(lib, "bmpc_biconvex_solve_batch_cone_frames_" + where)(C.byref(desc), C.byref(cone[0]), C.byref(cone[1]), *tail))
        return _lib.check(getattr(lib, "bmpc_biconvex_solve_batch_cone_" + where)(C.byref(desc), C.byref(cone), *tail))
    for kind, cost in (("blocks_", blocks), ("band_", band)):
        if cost is not None:
            return _lib.check(getattr(lib, "bmpc_biconvex_solve_batch_" + kind + where)(C.byref(desc), C.byref(cost), *tail))
    return _lib.check(getattr(lib, "bmpc_biconvex_solve_batch_" + where)(C.byref(desc), *tail))


def algorithmic_bytes_per_solve(H, E=4, per_problem_weights=False):
    """inputs (4E+10)H+18 doubles, outputs 18(H+1)+3EH+1 doubles
    (+ 9+9+3E+6+3 doubles when weights are per problem)."""
    n = (4 * E + 10) * H + 18 + 18 * (H + 1) + 3 * E * H + 1
    if per_problem_weights:
        n += 9 + 9 + 3 * E + 6 + 3
    return 8 * n


class DeviceBatch:
    """A problems.Batch resident on one GPU, harness form (the kernel applies create_cost_X /
    create_cost_F / create_bound_constraints itself) or, with raw=, the raw form."""

    def __init__(self, batch, device="cuda", num_iters=10, maxit=150, tol=1e-5, exit_tol=1e-3,
                 beta=1.5, mu=None, keep_hist=False, precision="f64", plan=None, raw=None, cone=None, plan_bounds=False):
        """plan: a plan_batch.DevicePlan whose tensors (cnt_plan, dt, X_nom, X_ter, x_init) are used in place of the
        batch's host arrays -- inputs built on the GPU never leave HBM.
        plan_bounds: the plan carries the kinematic bounds too, per problem and knot (plan.bounds (B, H, 6), sbounds = 6 H: an
        acyclic_batch.DeviceAcyclicPlan, whose bounds come from the motion's table); False: the batch's host array.
        raw: dict(Qx, qx, lbx, ubx, Qf[, qf][, Qx_blk][, Qf_blk]) -- the raw cost / bound form (solve_host explains it); with
        Qx_blk / Qf_blk the per-knot block costs, through bmpc_biconvex_solve_batch_blocks_device; with Qx_off / Qf_off the costs
        between neighbouring knots, through bmpc_biconvex_solve_batch_band_device
        cone: dict(projection="reference" | "euclidean", mu=None | array (1 or B, H, E)[, normals=array (1 or B, H, E, 3)]) -- the force
        step's projection, per-foot friction coefficients and contact normals, through bmpc_biconvex_solve_batch_cone_device or, with
        normals, bmpc_biconvex_solve_batch_cone_frames_device (solve_host explains it).  normals may be a contiguous float64 torch
        tensor on the batch's device -- plan_batch.DevicePlan(terrain=...).normals: it is used in place, no copy, no host trip"""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceBatch needs a GPU: no CPU fallback exists for the solve")
        self.torch = torch
        self.batch = batch
        self.device = torch.device(device)
        self.num_iters = num_iters
        B, H, E = batch.B, batch.H, batch.E
        f64 = torch.float64

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)

        if plan is None:
            self.t = dict(cnt_plan=up(batch.cnt_plan), dt=up(batch.dt), x_init=up(batch.x_init),
                          X_nom=up(batch.X_nom), X_ter=up(batch.X_ter))
        else:
            assert plan.B == B and plan.H == H
            self.t = dict(cnt_plan=plan.cnt_plan, dt=plan.dt, x_init=plan.inp["x_init"], X_nom=plan.X_nom, X_ter=plan.X_ter)
        self.blocks = None
        self.band = None
        if raw is None:
            if plan_bounds and (plan is None or tuple(plan.bounds.shape) != (B, H, 6)):
                raise ValueError("plan_bounds needs a plan with bounds (%d, %d, 6)" % (B, H))
            self.t.update(W_X=up(batch.W_X), W_X_ter=up(batch.W_X_ter), W_F=up(batch.W_F), bounds=plan.bounds if plan_bounds else up(batch.bounds))
        elif plan_bounds:
            raise ValueError("plan_bounds is for the harness form: the raw form takes lbx / ubx")
        else:
            for k in ("X_nom", "X_ter"):
                del self.t[k]
            for k in ("Qx", "qx", "lbx", "ubx", "Qf", "qf"):
                if raw.get(k) is not None and not (k in ("Qx", "Qf") and raw.get(k + "_blk") is not None):
                    assert np.shape(raw[k]) == (B, 3 * E * H if k in ("Qf", "qf") else 9 * (H + 1)), k
                    self.t[k] = up(raw[k])
            self.tb = {k: up(raw[k]) for k in ("Qx_blk", "Qf_blk") if raw.get(k) is not None}
            self.tk = {k: up(raw[k]) for k in ("Qx_off", "Qf_off") if raw.get(k) is not None}
            self.blocks = _cost_ext("blk", B, H, E, self.tb.get("Qx_blk"), self.tb.get("Qf_blk"), lambda t: t.data_ptr())
            if self.tb and self.tk:
                raise ValueError(_COMBINED)
            self.band = _cost_ext("off", B, H, E, self.tk.get("Qx_off"), self.tk.get("Qf_off"), lambda t: t.data_ptr())

        self.t_cone = []      # (the coefficients and the normals on the device)

        def up_cone(a):
            if isinstance(a, torch.Tensor):      # already in HBM (plan_batch.DevicePlan.normals): taken as it is, no copy
                index = lambda dev: torch.cuda.current_device() if dev.index is None else dev.index      # noqa: E731
                same = a.device.type == self.device.type and index(a.device) == index(self.device)
                if not same or a.dtype != f64 or not a.is_contiguous():
                    raise ValueError("cone: a torch tensor must be contiguous float64 on the batch's device %s, got %s on %s%s"
                                     % (self.device, a.dtype, a.device, "" if a.is_contiguous() else ", not contiguous"))
                self.t_cone.append(a)
            else:
                self.t_cone.append(up(a))
            return self.t_cone[-1].data_ptr()
        self.cone = _cone_ext(cone, B, H, E, up_cone)
        if cone is not None and cone.get("mu") is not None:
            self.t_mu = self.t_cone[0]
        self.X = torch.empty((B, 9 * (H + 1)), dtype=f64, device=self.device)
        self.F = torch.empty((B, 3 * E * H), dtype=f64, device=self.device)
        self.P = torch.empty((B, 9 * (H + 1)), dtype=f64, device=self.device)
        self.L_x = torch.full((B,), L0_X, dtype=f64, device=self.device)
        self.L_f = torch.full((B,), L0_F, dtype=f64, device=self.device)
        self.dyn_viol = torch.zeros(B, dtype=f64, device=self.device)
        self.stats = torch.zeros((B, NSTATS), dtype=torch.int32, device=self.device)
        self.hist = torch.full((B, max(num_iters, 1)), float("nan"), dtype=f64,
                               device=self.device) if keep_hist else None
        # with keep_hist the solve also leaves its discrete path per ADMM iteration (bmpc_batch_t.trace; -1 where none ran)
        self.trace = torch.full((B, max(num_iters, 1), 4), -1, dtype=torch.int32, device=self.device) if keep_hist else None
        d = _lib.Batch()
        _lib.lib().bmpc_batch_defaults(C.byref(d))
        _solver_fields(d, batch, num_iters, maxit, tol, exit_tol, beta, mu)
        d.precision = {"f64": 0, "f32": 1}[precision]
        d.raw = 0 if raw is None else 1
        d.cold_start = 1
        for k, v in self.t.items():
            setattr(d, k, v.data_ptr())
        if raw is None:
            d.sW_X, d.sW_X_ter = _stride(batch.W_X), _stride(batch.W_X_ter)
            d.sW_F, d.sbounds = _stride(batch.W_F), 6 * H if plan_bounds else _stride(batch.bounds)
        d.X, d.F, d.P = self.X.data_ptr(), self.F.data_ptr(), self.P.data_ptr()
        d.L_x, d.L_f = self.L_x.data_ptr(), self.L_f.data_ptr()
        d.dyn_viol, d.stats = self.dyn_viol.data_ptr(), self.stats.data_ptr()
        d.hist = self.hist.data_ptr() if keep_hist else None
        d.trace = self.trace.data_ptr() if keep_hist else None
        self.desc = d

    def set_warm_start(self, X, F, P, L_x=None, L_f=None):
        """set_warm_start_vars for the whole batch; the next solve() starts from these."""
        torch = self.torch
        self.X.copy_(torch.as_tensor(np.asarray(X), dtype=torch.float64))
        self.F.copy_(torch.as_tensor(np.asarray(F), dtype=torch.float64))
        self.P.copy_(torch.as_tensor(np.asarray(P), dtype=torch.float64))
        self.L_x.fill_(L0_X) if L_x is None else self.L_x.copy_(torch.as_tensor(np.asarray(L_x)))
        self.L_f.fill_(L0_F) if L_f is None else self.L_f.copy_(torch.as_tensor(np.asarray(L_f)))
        self.desc.cold_start = 0

    def cold_start(self, carry_step_constants=False):
        """Every solve starts as KinoDynMP::set_warm_starts does (kino_dyn.cpp:83-99): X = tile(x_init), F = 0, P = 0.
        carry_step_constants=False: with the constructor's FISTA constants too (a fresh KinoDynMP per problem: independent batch
        elements).  True: L_x / L_f stay what the previous solve left (or set_step_constants set) -- the reference never resets
        FISTA's L_ between the optimize calls of one object (fista.hpp:52), so this is the mode for successive replans of the same
        rollouts."""
        self.desc.cold_start = 2 if carry_step_constants else 1

    def set_step_constants(self, L_x, L_f):
        torch = self.torch
        self.L_x.copy_(torch.as_tensor(np.broadcast_to(np.asarray(L_x, dtype=np.float64), self.L_x.shape).copy()))
        self.L_f.copy_(torch.as_tensor(np.broadcast_to(np.asarray(L_f, dtype=np.float64), self.L_f.shape).copy()))

    def solve(self):
        """Asynchronous: one launch on torch's current stream."""
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        if self.hist is not None:      # rows of ADMM iterations that do not run keep their NaN / -1
            self.hist.fill_(float("nan"))
            self.trace.fill_(-1)
        _launch(self.desc, self.blocks, self.band, stream, cone=self.cone)

    def results(self):
        self.torch.cuda.synchronize(self.device)
        out = dict(X=self.X.cpu().numpy(), F=self.F.cpu().numpy(), P=self.P.cpu().numpy(),
                   L_x=self.L_x.cpu().numpy(), L_f=self.L_f.cpu().numpy(),
                   dyn_viol=self.dyn_viol.cpu().numpy(), stats=self.stats.cpu().numpy().astype(np.int64))
        if self.hist is not None:
            out["hist"] = self.hist.cpu().numpy()
            out["trace"] = self.trace.cpu().numpy().astype(np.int64)
        return out


def solve_host(batch, num_iters=10, maxit=150, tol=1e-5, exit_tol=1e-3, beta=1.5, mu=None,
               warm=None, L_x=None, L_f=None, raw=None, keep_hist=False, precision="f64", cert_phases=False, cone=None):
    """numpy in / numpy out through bmpc_biconvex_solve_batch_host (copies in, one launch,
    copies out).  warm = (X, F, P) or None for a cold start.  raw = dict(Qx,qx,lbx,ubx,Qf[,qf])
    switches to the raw cost/bound form; with Qx_blk (1 or B, H + 1, 9, 9) and / or Qf_blk (1 or B, H, 3E, 3E) in it that side's
    cost is block-diagonal per knot (symmetric blocks; a leading dimension of 1: shared by the batch) and its Qx / Qf may be left
    out (bmpc_biconvex_solve_batch_blocks_host).  With Qx_off (1 or B, H, 9) and / or Qf_off (1 or B, H - 1, 3E) in it, Q has the
    weight off[t][i] between component i of knots t and t + 1 beside its diagonal Qx / Qf -- force-rate and momentum-rate costs
    (bmpc_biconvex_solve_batch_band_host); not together with blocks.  cert_phases: also return "cert_phases" (B, 2), the force and
    motion phases per problem that ran the certified FISTA loop from their first iteration (bmpc_batch_t.cert_phases; -1 where the
    kernel records none).  cone = dict(projection="euclidean", mu=None | array (1 or B, H, E)): the force step projects onto the
    friction cone |f_xy| <= mu f_z (the nearest point; the default, "reference", is the reference's "SoC" step) with a coefficient per
    problem, knot and foot (a leading dimension of 1: shared by the batch; None: the scalar mu) -- either form, fp64, H + 1 <= 64, not
    together with blocks or band costs (bmpc_biconvex_solve_batch_cone_host).  With normals=array (1 or B, H, E, 3) in it, unit vectors in
    the world frame, the cone of a contact is about its surface normal instead of world z: |f - (n.f) n| <= mu n.f
    (bmpc_biconvex_solve_batch_cone_frames_host; "euclidean" only)."""
    B, H, E = batch.B, batch.H, batch.E
    nx, nf = 9 * (H + 1), 3 * E * H
    keep = []

    def f64(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return a

    blocks = band = None
    d = _lib.Batch()
    _lib.lib().bmpc_batch_defaults(C.byref(d))
    _solver_fields(d, batch, num_iters, maxit, tol, exit_tol, beta, mu)
    d.precision = {"f64": 0, "f32": 1}[precision]
    for k in ("cnt_plan", "dt", "x_init"):
        setattr(d, k, f64(getattr(batch, k)).ctypes.data)
    if raw is None:
        d.raw = 0
        for k in ("W_X", "W_X_ter", "W_F", "bounds", "X_nom", "X_ter"):
            setattr(d, k, f64(getattr(batch, k)).ctypes.data)
        d.sW_X, d.sW_X_ter = _stride(batch.W_X), _stride(batch.W_X_ter)
        d.sW_F, d.sbounds = _stride(batch.W_F), _stride(batch.bounds)
    else:
        d.raw = 1
        blocks, band = (_cost_ext(kind, B, H, E, *(None if raw.get(k) is None else f64(raw[k]) for k in ("Qx_" + kind, "Qf_" + kind)),
                                  put=lambda a: a.ctypes.data) for kind in ("blk", "off"))
        if blocks is not None and band is not None:
            raise ValueError(_COMBINED)
        for k in ("Qx", "qx", "lbx", "ubx", "Qf"):
            if raw.get(k) is None and k in ("Qx", "Qf") and raw.get(k + "_blk") is not None:
                continue
            a = f64(raw[k])
            assert a.shape == (B, nf if k == "Qf" else nx), k
            setattr(d, k, a.ctypes.data)
        if raw.get("qf") is not None:
            d.qf = f64(raw["qf"]).ctypes.data
    if warm is None:
        d.cold_start = 1
        X, F, P = np.zeros((B, nx)), np.zeros((B, nf)), np.zeros((B, nx))
    else:
        d.cold_start = 0
        X, F, P = (np.array(a, dtype=np.float64, order="C").reshape(B, -1) for a in warm)
    Lx = np.full(B, L0_X) if L_x is None else np.array(L_x, dtype=np.float64).reshape(B)
    Lf = np.full(B, L0_F) if L_f is None else np.array(L_f, dtype=np.float64).reshape(B)
    viol = np.zeros(B)
    stats = np.zeros((B, NSTATS), dtype=np.int32)
    hist = np.full((B, max(num_iters, 1)), np.nan) if keep_hist else None
    d.X, d.F, d.P = X.ctypes.data, F.ctypes.data, P.ctypes.data
    d.L_x, d.L_f, d.dyn_viol, d.stats = Lx.ctypes.data, Lf.ctypes.data, viol.ctypes.data, stats.ctypes.data
    trace = np.full((B, max(num_iters, 1), 4), -1, dtype=np.int32) if keep_hist else None
    d.hist = hist.ctypes.data if keep_hist else None
    d.trace = trace.ctypes.data if keep_hist else None
    certn = np.full((B, 2), -1, dtype=np.int32) if cert_phases else None
    d.cert_phases = certn.ctypes.data if cert_phases else None
    _launch(d, blocks, band, cone=_cone_ext(cone, B, H, E, lambda a: f64(a).ctypes.data))
    out = dict(X=X, F=F, P=P, L_x=Lx, L_f=Lf, dyn_viol=viol, stats=stats.astype(np.int64))
    if cert_phases:
        out["cert_phases"] = certn.astype(np.int64)
    if keep_hist:
        out["hist"] = hist
        out["trace"] = trace.astype(np.int64)
    return out
