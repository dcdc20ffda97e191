"""The policy network's forward pass (include/ext/bunmpc_policy.h): the reference's `GoalConditionedPolicyNet`
(`ISL/examples/iterative_algorithm/networks.py`) in eval() mode as one kernel launch on rows that are device tensors already -- the `x` of
`DeviceDatabase.batch(index)`, or the states and goals of a batch of rollouts with the normalisation of `simulation.py:1702-1710` folded in:

    net = PolicyNet.from_state_dict(torch.load(path)["network"])       # or .from_module(m) / .from_arrays(W, b)
    policy = DevicePolicy(net, "cuda")                                 # packs and uploads once
    action = policy.forward(x)                                         # (n, out) float64; kernels on torch's current stream, no synchronisation
    action, tau = policy.act(states, goals, norm=DevicePolicy.norm_of(db), q=q, v=v, kp=2.0, kd=0.1, action_type="pd_target")
    err = policy.l1_rows(x, y)                                         # (n,) the rows' summands of nn.L1Loss(reduction="sum")

`host_forward` is the same function in numpy and the specification: the device result equals it in every bit.  The training step, and this class on the
weights being trained, are bunmpc_amd/policy_train.py::DeviceTrainer."""
import ctypes as C
import re

import numpy as np

from . import _lib, _lib_policy

PAD = _lib_policy.PAD


# ---- the host twin -------------------------------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """fmaf on float32 arrays, correctly rounded: the product is exact in float64 (48 bits), the sum is rounded to odd there (TwoSum
    gives the error's sign), and 53 bits rounded to odd, then to the nearest float32 is the nearest float32 of the exact value."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1).astype(bool)
        nudge = np.isfinite(s) & (e != 0) & ~odd
        s = np.where(nudge, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def pad(v):
    return (v + PAD - 1) // PAD * PAD


class PolicyNet:
    """The arrays of one network on the host, float32 as torch holds them.  W[l] (N_l, K_l), b[l] (N_l,) for l = 0 .. n_layers (the last is
    the output layer); bn[l] = (gamma, beta, running_mean, running_var) per hidden layer, or bn = None."""

    def __init__(self, W, b, bn=None, eps=1e-5):
        f32 = lambda v: np.ascontiguousarray(_numpy(v), dtype=np.float32)      # noqa: E731
        self.W, self.b = [f32(w) for w in W], [f32(v) for v in b]
        self.bn = None if bn is None else [tuple(f32(v) for v in layer) for layer in bn]
        self.eps = float(eps)
        self.n_layers = len(self.W) - 1
        if self.n_layers < 1 or len(self.b) != len(self.W):
            raise ValueError("a network has at least one hidden layer and a bias per layer: got %d W, %d b" % (len(self.W), len(self.b)))
        self.n_in, self.n_hidden, self.n_out = self.W[0].shape[1], self.W[0].shape[0], self.W[-1].shape[0]
        for l, (w, v) in enumerate(zip(self.W, self.b)):
            want = (self.n_out if l == self.n_layers else self.n_hidden, self.n_in if l == 0 else self.n_hidden)
            if w.shape != want or v.shape != want[:1]:
                raise ValueError("layer %d: W %s and b %s expected, got %s and %s" % (l, want, want[:1], w.shape, v.shape))
        if self.bn is not None and (len(self.bn) != self.n_layers or any(len(g) != 4 or any(v.shape != (self.n_hidden,) for v in g) for g in self.bn)):
            raise ValueError("bn: (gamma, beta, running_mean, running_var) of %d values for each of the %d hidden layers" % (self.n_hidden, self.n_layers))

    batch_norm = property(lambda self: self.bn is not None)
    dims = property(lambda self: (self.n_in, self.n_hidden, self.n_layers, self.n_out, int(self.batch_norm)))

    @classmethod
    def from_arrays(cls, W, b, bn=None, eps=1e-5):
        return cls(W, b, bn, eps)

    @classmethod
    def from_state_dict(cls, sd, eps=1e-5):
        """the reference's keys net.<i>.weight / .bias, and .running_mean / .running_var on its BatchNorm1d entries (torch tensors or
        numpy); eps is not in a state_dict: BatchNorm1d's default unless given"""
        entries = {}
        for key, v in sd.items():
            m = re.fullmatch(r"net\.(\d+)\.(\w+)", key)
            if not m:
                raise ValueError("not a key of GoalConditionedPolicyNet: %r" % key)
            entries.setdefault(int(m.group(1)), {})[m.group(2)] = _numpy(v)
        linear = [e for _, e in sorted(entries.items()) if "running_mean" not in e]
        norms = [e for _, e in sorted(entries.items()) if "running_mean" in e]
        bn = [(e["weight"], e["bias"], e["running_mean"], e["running_var"]) for e in norms] or None
        return cls([e["weight"] for e in linear], [e["bias"] for e in linear], bn, eps)

    @classmethod
    def from_module(cls, module):
        """a GoalConditionedPolicyNet (or any module with its `net` Sequential); with BatchNorm1d it must be in eval() mode"""
        norms = [m for m in module.modules() if type(m).__name__ == "BatchNorm1d"]
        if norms and module.training:
            raise ValueError("a network with BatchNorm1d is evaluated with its running statistics: call .eval() first")
        return cls.from_state_dict(module.state_dict(), eps=norms[0].eps if norms else 1e-5)

    def scale_shift(self, l):
        """step c's s, t of hidden layer l: float64 arithmetic on the float32 arrays, rounded once"""
        gamma, beta, mean, var = (v.astype(np.float64) for v in self.bn[l])
        s = gamma / np.sqrt(var + self.eps)
        return s.astype(np.float32), (beta - mean * s).astype(np.float32)


def _numpy(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


def host_input(net, x=None, state=None, goal=None, mean=None, std=None):
    """step a: (n, n_in) float32"""
    if (x is None) == (state is None and goal is None):
        raise ValueError("one input form: x, or state and goal")
    if x is None:
        v = np.hstack((np.asarray(state, np.float64), np.asarray(goal, np.float64)))
        if (mean is None) != (std is None):
            raise ValueError("mean and std go together")
        if mean is not None:
            with np.errstate(all="ignore"):
                v = (v - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    else:
        if mean is not None or std is not None:
            raise ValueError("mean / std go with the state, goal form")
        v = np.asarray(x, np.float64)
    if v.ndim != 2 or v.shape[1] != net.n_in:
        raise ValueError("input rows of %d expected, got %s" % (net.n_in, v.shape))
    with np.errstate(all="ignore"):
        return v.astype(np.float32)


def host_layers(net, a):
    """steps b to d on (n, n_in) float32 rows: (n, n_out) float32"""
    a = np.asarray(a, np.float32)
    for l in range(net.n_layers + 1):
        W, K = net.W[l], net.W[l].shape[1]
        acc = np.broadcast_to(net.b[l], (a.shape[0], W.shape[0])).copy()
        zero = np.float32(0)
        for k in range(pad(K)):
            acc = fma32(W[:, k], a[:, k:k + 1], acc) if k < K else fma32(zero, zero, acc)
        if l < net.n_layers:
            if net.batch_norm:
                s, t = net.scale_shift(l)
                acc = fma32(acc, s, t)
            with np.errstate(invalid="ignore"):
                acc = np.where(acc <= 0, np.float32(0), acc)
        a = acc
    return a


def host_forward(net, x=None, state=None, goal=None, mean=None, std=None):
    """the function of include/ext/bunmpc_policy.h, steps a to d: (n, n_out) float32"""
    return host_layers(net, host_input(net, x, state, goal, mean, std))


def host_tau(action, q, v, kp, kd, action_type):
    """step e's tau (n, 12) float64 from the float32 action, q (n, 19), v (n, 18)"""
    a = np.asarray(action, np.float32).astype(np.float64)
    if action_type == "torque":
        return a.copy()
    qj, vj = np.asarray(q, np.float64)[:, 7:19], np.asarray(v, np.float64)[:, 6:18]
    with np.errstate(all="ignore"):
        if action_type == "pd_target":
            return kp * (a - qj) - kd * vj
        if action_type == "structured":
            return (a[:, 0:12] + kp * (a[:, 12:24] - qj)) + kd * (a[:, 24:36] - vj)
    raise ValueError("action_type must be torque, pd_target or structured, got %r" % (action_type,))


def host_l1_rows(action, label):
    """step e's err (n,) float64: the sum over j ascending"""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(action, np.float32).astype(np.float64) - np.asarray(label, np.float64).astype(np.float32).astype(np.float64))
        e = np.zeros(d.shape[0])
        for j in range(d.shape[1]):
            e = e + d[:, j]
    return e


# ---- the packed image ------------------------------------------------------------------------------------------------------------------

def _desc(net):
    d = _lib_policy.PolicyNetDesc()
    d.n_in, d.n_hidden, d.n_layers, d.n_out, d.batch_norm = net.dims
    d.packed_bytes = _lib_policy.lib().bmpc_policy_packed_bytes(*net.dims)
    if d.packed_bytes < 0:
        raise ValueError("n_in, n_hidden in [1, %d], 1 to %d hidden layers, n_out in [1, %d]; got %d, %d, %d, %d"
                         % (_lib_policy.MAX_WIDTH, _lib_policy.MAX_LAYERS, _lib_policy.MAX_OUT, net.n_in, net.n_hidden, net.n_layers, net.n_out))
    return d


def pack(net):
    """the packed image of `net` as the library's packer writes it: a float32 array"""
    d = _desc(net)
    image = np.zeros(d.packed_bytes // 4 + 4, np.float32)
    image = image[(-image.ctypes.data % 16) // 4:][:d.packed_bytes // 4]      # 16-byte aligned
    d.packed = image.ctypes.data
    w = _lib_policy.PolicyWeights()
    w.eps = net.eps
    for l in range(net.n_layers + 1):
        w.W[l], w.b[l] = net.W[l].ctypes.data, net.b[l].ctypes.data
        if net.batch_norm and l < net.n_layers:
            w.gamma[l], w.beta[l], w.running_mean[l], w.running_var[l] = (v.ctypes.data for v in net.bn[l])
    _lib.check(_lib_policy.lib().bmpc_policy_pack_host(C.byref(d), C.byref(w)))
    return image


def unpack(dims, image):
    """[(W (Np, Kp), b (Np,), s, t (Np,) or None)] per layer of an image of a network of `dims` = (n_in, n_hidden, n_layers, n_out,
    batch_norm), padding included: the layout of the header's packer, read backwards"""
    n_in, n_hidden, n_layers, n_out, batch_norm = dims
    out, at = [], 0
    for l in range(n_layers + 1):
        Kp, Np = pad(n_in if l == 0 else n_hidden), pad(n_out if l == n_layers else n_hidden)
        tiles = np.asarray(image[at:at + Np * Kp]).reshape(Np // 16, Kp // 16, 4, 16, 4)      # jt, kq, lane / 16, lane % 16, i
        W = tiles.transpose(0, 3, 1, 4, 2).reshape(Np, Kp)                                    # j = 16 jt + lane % 16, k = 16 kq + 4 i + lane / 16
        at += Np * Kp
        rest = [image[at + i * Np:at + (i + 1) * Np] for i in range(3 if batch_norm and l < n_layers else 1)]
        at += len(rest) * Np
        out.append((W, rest[0], rest[1] if len(rest) > 1 else None, rest[2] if len(rest) > 1 else None))
    if at != len(image):
        raise ValueError("an image of %d floats expected, got %d" % (at, len(image)))
    return out


# ---- the device ------------------------------------------------------------------------------------------------------------------------

def device_rows(device, name, t, width, n=None):
    """(address, row stride) of a float64 tensor (n, width) on `device` (a torch.device with its index, as a tensor's .device is) whose
    rows are contiguous; any row stride >= width is used in place.  The argument check of DevicePolicy and of policy_train.DeviceTrainer."""
    if str(t.dtype) != "torch.float64" or t.device != device:
        raise ValueError("%s: a float64 tensor on %s is expected, got %s on %s" % (name, device, t.dtype, t.device))
    if t.dim() != 2 or t.shape[1] != width or (n is not None and t.shape[0] != n):
        raise ValueError("%s: expected shape (%s, %d), got %s" % (name, "n" if n is None else n, width, tuple(t.shape)))
    if t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < width):
        raise ValueError("%s: rows must be contiguous and not overlap: strides %s" % (name, tuple(t.stride())))
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else width)


class DevicePolicy:
    def __init__(self, net, device="cuda"):
        import torch
        self.torch, self.device, self.net = torch, torch.device(device), net
        self.desc = _desc(net)
        self.packed = torch.from_numpy(pack(net).copy()).to(self.device)
        self.desc.packed = self.packed.data_ptr()
        self.tile = _lib_policy.lib().bmpc_policy_tile()

    def _rows(self, name, t, width, n=None):
        return device_rows(self.packed.device, name, t, width, n)

    def _launch(self, r):
        if r.n:      # (empty tensors have no address to pass)
            _lib.check(_lib_policy.lib().bmpc_policy_forward_device(C.byref(self.desc), C.byref(r), C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)))

    def _out(self, *shape):
        return self.torch.empty(shape, dtype=self.torch.float64, device=self.device)

    def forward(self, x):
        """x (n, n_in) float64, assembled and normalised already (DeviceDatabase.batch's x): the action (n, n_out) float64"""
        r = _lib_policy.PolicyRows()
        r.x, r.x_stride = self._rows("x", x, self.net.n_in)
        r.n = x.shape[0]
        action = self._out(r.n, self.net.n_out)
        r.action = action.data_ptr()
        self._launch(r)
        return action

    def act(self, states, goals, norm=None, q=None, v=None, kp=0.0, kd=0.0, action_type="pd_target"):
        """states (n, 43), goals (n, n_in - 43) float64, used in place whatever their row strides; norm = (mean, std), (n_in,) device
        tensors each (norm_of), or None; q (n, 19), v (n, 18) the measured configuration and velocity (two views of a [q | v] buffer are
        fine).  Returns (action (n, n_out), tau (n, 12)) as simulation.py:1714-1731 turns the action into a torque; tau is None where q, v
        are not given and the type needs them."""
        if action_type not in _lib_policy.ACTION_TYPE:
            raise ValueError("action_type must be torque, pd_target or structured, got %r" % (action_type,))
        r = _lib_policy.PolicyRows()
        r.n = n = states.shape[0]
        r.state, r.state_stride = self._rows("states", states, _lib_policy.STATE_WIDTH)
        r.goal, r.goal_stride = self._rows("goals", goals, self.net.n_in - _lib_policy.STATE_WIDTH, n)
        if norm is not None:
            mean, std = (t.contiguous() for t in norm)
            r.mean, r.std = self._rows("mean", mean[None], self.net.n_in)[0], self._rows("std", std[None], self.net.n_in)[0]
        action, tau = self._out(n, self.net.n_out), None
        r.action = action.data_ptr()
        if action_type == "torque" or (q is not None and v is not None):
            tau = self._out(n, _lib_policy.TAU_WIDTH)
            r.tau, r.action_type, r.kp, r.kd = tau.data_ptr(), _lib_policy.ACTION_TYPE[action_type], float(kp), float(kd)
            if action_type != "torque":
                r.q, r.q_stride = self._rows("q", q, _lib_policy.Q_WIDTH, n)
                r.v, r.v_stride = self._rows("v", v, _lib_policy.V_WIDTH, n)
        self._launch(r)
        return action, tau

    def l1_rows(self, x, y):
        """err (n,): row i's sum over j of |net(x[i])[j] - float32(y[i][j])|, the summands of the reference's validation loss"""
        r = _lib_policy.PolicyRows()
        r.x, r.x_stride = self._rows("x", x, self.net.n_in)
        r.n = n = x.shape[0]
        r.label, r.label_stride = self._rows("y", y, self.net.n_out, n)
        err = self._out(n)
        r.err = err.data_ptr()
        self._launch(r)
        return err

    @staticmethod
    def norm_of(db):
        """(mean, std) of a DeviceDatabase's current goal type as one (43 + goal width,) device tensor each: [states | goal]; None where
        the data set does not normalise.  calc_input_mean_std() must have run."""
        stats = db.get_database_mean_std()
        if stats is None:
            return None
        if stats[0] is None:
            raise ValueError("norm_of: calc_input_mean_std() has not run")
        torch = db.torch
        wide = lambda v, like: v if torch.is_tensor(v) else torch.full((db.desc.w_vc,), float(v), dtype=like.dtype, device=like.device)      # noqa: E731
        return torch.cat((stats[0], wide(stats[2], stats[0]))), torch.cat((stats[1], wide(stats[3], stats[1])))
