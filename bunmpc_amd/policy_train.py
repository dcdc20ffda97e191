"""The policy network's training step (include/ext/bunmpc_policy_train.h): the loop of the reference's
`behavioral_cloning_train.py:123-149` -- `GoalConditionedPolicyNet` in train() mode, `nn.L1Loss()`, `loss.backward()`, `torch.optim.Adam(lr)` --
as 3 n_layers + 4 kernel launches per step on rows that are device tensors already, and one more that rewrites the packed image of
`DevicePolicy` on the device:

    trainer = DeviceTrainer(PolicyNet.from_module(network.eval()), "cuda", lr=0.002)
    loss = trainer.step(*db.batch(index))                              # a float64 device scalar; no synchronisation
    trainer = DeviceTrainer(net, "cuda", keep_grads=True)              # gradients are kept only on request:
    norm = sum(g.square().sum() for _, g in trainer.grads().arrays()).sqrt()      # the last step's, device tensors (gradient-norm logging)
    history = trainer.fit(db, n_epoch=150, batch_size=256)             # [(train_loss, valid_loss)] per epoch, one host read per epoch
    action = trainer.policy.forward(x)                                 # the same DevicePolicy, on the current weights
    torch.save({"network": trainer.state_dict()}, path)                # the reference's keys; trainer.net() is the PolicyNet

`host_step` is the same function in numpy and the specification: the device's loss, gradients, parameters, Adam moments and running
statistics equal it in every bit, whatever the launch geometry, so a training run reproduces across machines."""
import ctypes as C

import numpy as np

from . import _lib, _lib_policy, _lib_policy_train, policy
from .policy import PolicyNet, fma32

PAD = _lib_policy_train.PAD
BETA1, BETA2, ADAM_EPS, MOMENTUM = 0.9, 0.999, 1e-8, 0.1
_F = np.float32
_ZERO, _ONE = _F(0), _F(1)


# ---- the host twin -------------------------------------------------------------------------------------------------------------------

def sqrt32(a):
    """IEEE float32 sqrt: the float64 root rounded once more (53 >= 2 * 24 + 2 bits: the second rounding changes nothing)"""
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(a, _F).astype(np.float64)).astype(_F)


def div32(a, b):
    """IEEE float32 divide, by way of float64 as sqrt32"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, _F).astype(np.float64) / np.asarray(b, _F).astype(np.float64)).astype(_F)


def chain(a, b=None):
    """the one reduction rule over axis 0: s = +0; s = fmaf(a[i], b[i], s) for i ascending (b = None: a plain term, a[i] * 1), then the +0
    terms that pad the count to a multiple of PAD"""
    a = np.asarray(a, _F)
    s = np.zeros(np.broadcast_shapes(a.shape[1:], () if b is None else np.shape(b)[1:]), _F)
    for i in range(a.shape[0]):
        s = fma32(a[i], _ONE if b is None else b[i], s)
    if a.shape[0] % PAD:
        s = fma32(_ZERO, _ZERO, s)
    return s


class Params:
    """W[l], b[l] for l = 0 .. n_layers and gamma[l], beta[l] per hidden layer (None without BatchNorm): the parameters, their gradients
    or one of Adam's moments"""

    def __init__(self, W, b, gamma=None, beta=None):
        self.W, self.b, self.gamma, self.beta = list(W), list(b), None if gamma is None else list(gamma), None if beta is None else list(beta)

    def arrays(self):
        """(name, array) in the order of torch's parameters()"""
        for l in range(len(self.W)):
            yield "W%d" % l, self.W[l]
            yield "b%d" % l, self.b[l]
            if self.gamma is not None and l < len(self.gamma):
                yield "gamma%d" % l, self.gamma[l]
                yield "beta%d" % l, self.beta[l]

    def map(self, fn, *others):
        pick = lambda q, name, l: getattr(q, name)[l]      # noqa: E731
        out = {name: None if getattr(self, name) is None else [fn(v, *(pick(o, name, l) for o in others)) for l, v in enumerate(getattr(self, name))]
               for name in ("W", "b", "gamma", "beta")}
        return Params(**out)


class TrainState:
    """what one step reads and writes: the parameters p, Adam's moments m and v (all Params of float32 arrays) and the running statistics"""

    def __init__(self, p, m=None, v=None, running_mean=None, running_var=None, eps=1e-5):
        f32 = lambda a: np.array(a, dtype=_F)      # noqa: E731  (a copy)
        self.p = p.map(f32)
        self.m = self.p.map(np.zeros_like) if m is None else m.map(f32)
        self.v = self.p.map(np.zeros_like) if v is None else v.map(f32)
        self.running_mean = None if running_mean is None else [f32(a) for a in running_mean]
        self.running_var = None if running_var is None else [f32(a) for a in running_var]
        self.eps = float(eps)
        if (self.p.gamma is None) != (self.running_mean is None):
            raise ValueError("gamma, beta and the running statistics go together")

    batch_norm = property(lambda self: self.p.gamma is not None)
    n_layers = property(lambda self: len(self.p.W) - 1)

    @classmethod
    def from_net(cls, net):
        bn = net.bn
        return cls(Params(net.W, net.b, None if bn is None else [g[0] for g in bn], None if bn is None else [g[1] for g in bn]),
                   running_mean=None if bn is None else [g[2] for g in bn], running_var=None if bn is None else [g[3] for g in bn], eps=net.eps)

    def net(self):
        bn = [(self.p.gamma[l], self.p.beta[l], self.running_mean[l], self.running_var[l]) for l in range(self.n_layers)] if self.batch_norm else None
        return PolicyNet.from_arrays(self.p.W, self.p.b, bn, self.eps)

    def copy(self):
        return TrainState(self.p, self.m, self.v, self.running_mean, self.running_var, self.eps)


def host_train_forward(state, x):
    """steps a to d in train() mode on x (n, n_in) float64.  Returns a dict: a (the layers' inputs a_0 .. a_L), xhat, invstd, mean, var
    (per hidden layer with BatchNorm), p (n, n_out) float32, and running_mean, running_var after the step."""
    with np.errstate(all="ignore"):
        a = np.asarray(x, np.float64).astype(_F)
        n, fn = a.shape[0], _F(a.shape[0])
        if state.batch_norm and n < 2:
            raise ValueError("BatchNorm in train() mode needs 2 rows at least")
        out = dict(a=[], xhat=[], invstd=[], mean=[], var=[], running_mean=[], running_var=[])
        for l in range(state.n_layers + 1):
            W, K = state.p.W[l], state.p.W[l].shape[1]
            out["a"].append(a)
            z = np.broadcast_to(state.p.b[l], (n, W.shape[0])).copy()
            for k in range(K):
                z = fma32(W[:, k], a[:, k:k + 1], z)
            if K % PAD:
                z = fma32(_ZERO, _ZERO, z)
            if l == state.n_layers:
                out["p"] = z
                break
            if state.batch_norm:
                mean = div32(chain(z), fn)
                d = z - mean
                var = div32(chain(d, d), fn)
                invstd = div32(_ONE, sqrt32(var + _F(state.eps)))
                xhat = d * invstd
                z = fma32(xhat, state.p.gamma[l], state.p.beta[l])
                mom, keep = _F(MOMENTUM), _ONE - _F(MOMENTUM)
                out["running_mean"].append(fma32(mom, mean, keep * state.running_mean[l]))
                out["running_var"].append(fma32(mom, div32(var * fn, fn - _ONE), keep * state.running_var[l]))
                for key, val in (("xhat", xhat), ("invstd", invstd), ("mean", mean), ("var", var)):
                    out[key].append(val)
            a = np.where(z <= 0, _ZERO, z)
        return out


def host_loss(p, y):
    """step e: the loss, float64"""
    with np.errstate(all="ignore"):
        y32 = np.asarray(y, np.float64).astype(_F)
        e = policy.host_l1_rows(p, y32)
        total = np.float64(0)
        for r in range(e.shape[0]):
            total = total + e[r]
        return total / np.float64(p.shape[0] * p.shape[1])


def host_backward(state, fwd, y):
    """step f from host_train_forward's dict: the gradients, a Params"""
    with np.errstate(all="ignore"):
        p, y32 = fwd["p"], np.asarray(y, np.float64).astype(_F)
        n, fn = p.shape[0], _F(p.shape[0])
        c = div32(_ONE, _F(n * p.shape[1]))
        t = p - y32
        dz = np.where(t > 0, c, np.where(t < 0, -c, np.where(t == 0, _ZERO, t))).astype(_F)
        L = state.n_layers
        g = Params([None] * (L + 1), [None] * (L + 1), [None] * L if state.batch_norm else None, [None] * L if state.batch_norm else None)
        for l in range(L, -1, -1):
            a = fwd["a"][l]
            g.b[l] = chain(dz)
            g.W[l] = chain(dz[:, :, None], a[:, None, :])
            if l == 0:
                break
            W = state.p.W[l]
            da = chain(W[:, None, :], dz.T[:, :, None])                    # over j: (n, K)
            du = np.where(a <= 0, _ZERO, da)
            if state.batch_norm:
                xhat = fwd["xhat"][l - 1]
                g.beta[l - 1], g.gamma[l - 1] = chain(du), chain(du, xhat)
                scale = state.p.gamma[l - 1] * fwd["invstd"][l - 1]
                mb, mg = div32(g.beta[l - 1], fn), div32(g.gamma[l - 1], fn)
                dz = fma32(-xhat, mg, du - mb) * scale
            else:
                dz = du
        return g


def bias_corrections(t):
    """Adam's two, float64, for the step count t = 1, 2, ..."""
    return 1.0 - BETA1 ** t, 1.0 - BETA2 ** t


def host_adam(p, g, m, v, lr, t):
    """step g on Params p, m, v with the gradients g at the count t: (p', m', v')"""
    bc1, bc2 = bias_corrections(t)
    w1, w2, b2 = _F(1.0 - BETA1), _F(1.0 - BETA2), _F(BETA2)
    step, root, eps = _F(lr / bc1), _F(np.sqrt(bc2)), _F(ADAM_EPS)
    with np.errstate(all="ignore"):
        m1 = m.map(lambda mq, gq: fma32(w1, gq - mq, mq), g)
        v1 = v.map(lambda vq, gq: fma32(w2 * gq, gq, b2 * vq), g)
        p1 = p.map(lambda q, mq, vq: fma32(-step, div32(mq, div32(sqrt32(vq), root) + eps), q), m1, v1)
    return p1, m1, v1


def host_step(state, x, y, lr, t):
    """the function of include/ext/bunmpc_policy_train.h: (state', loss, grads); `state` is left as it is"""
    fwd = host_train_forward(state, x)
    loss = host_loss(fwd["p"], y)
    g = host_backward(state, fwd, y)
    p, m, v = host_adam(state.p, g, state.m, state.v, lr, t)
    return TrainState(p, m, v, fwd["running_mean"] if state.batch_norm else None, fwd["running_var"] if state.batch_norm else None, state.eps), loss, g


def state_dict_arrays(net, num_batches_tracked=0):
    """{key: array} with the reference's keys (net.<i>.weight, ...), in the order of GoalConditionedPolicyNet.state_dict()"""
    out, i = {}, 0
    for l in range(net.n_layers + 1):
        out["net.%d.weight" % i], out["net.%d.bias" % i] = net.W[l], net.b[l]
        i += 1
        if l < net.n_layers:
            if net.batch_norm:
                for name, v in zip(("weight", "bias", "running_mean", "running_var"), net.bn[l]):
                    out["net.%d.%s" % (i, name)] = v
                out["net.%d.num_batches_tracked" % i] = np.asarray(num_batches_tracked, np.int64)
                i += 1
            i += 1      # the ReLU
    return out


# ---- the reference's loop ------------------------------------------------------------------------------------------------------------------

def fit_indices(n_rows, n_epoch, batch_size=256, n_train_frac=0.9, seed=0):
    """the rows of train_network's loop: a seeded random split into int(n_train_frac n_rows) training rows and the rest, and per epoch a new
    permutation of the training rows cut into batches of batch_size, the last short one dropped.  Returns ([[index per batch] per epoch],
    the validation rows)."""
    rng = np.random.default_rng(seed)
    split = rng.permutation(int(n_rows))
    n_train = int(n_train_frac * n_rows)
    train, valid = split[:n_train], split[n_train:]
    epochs = []
    for _ in range(n_epoch):
        order = train[rng.permutation(n_train)]
        epochs.append([order[i * batch_size:(i + 1) * batch_size] for i in range(n_train // batch_size)])
    return epochs, valid


class _Loop:
    """fit() over the three calls a trainer has: step(x, y) -> loss, l1_rows(x, y) -> the rows' summands, _read(values) -> one host array"""

    def fit(self, db, n_epoch, batch_size=256, n_train_frac=0.9, seed=0):
        """the loop of behavioral_cloning_train.py:104-158 on a data set with batch(index) and len(): per epoch one step per training batch,
        then the validation loss of the new weights in eval() mode over every validation row (mean |p - y| as nn.L1Loss takes it).  One host
        read per epoch.  Returns [(train_loss, valid_loss)] per epoch: the mean of the batches' losses, and NaN where there is no row."""
        epochs, valid = fit_indices(len(db), n_epoch, batch_size, n_train_frac, seed)
        history = []
        for batches in epochs:
            losses = [self.step(*db.batch(index)) for index in batches]
            errs = [self.l1_rows(*db.batch(valid[i:i + batch_size])) for i in range(0, len(valid), batch_size)]
            values = self._read(losses, errs)
            nb = len(losses)
            with np.errstate(all="ignore"):
                train = np.mean(values[:nb]) if nb else np.nan
                val = np.sum(values[nb:]) / (len(valid) * self.n_out) if len(valid) else np.nan
            history.append((float(train), float(val)))
        return history


class HostTrainer(_Loop):
    """the twin as a trainer: host_step on numpy rows, for tests and for the loop's specification"""

    def __init__(self, net, lr=0.002):
        self.state, self.lr, self.t, self.n_out = TrainState.from_net(net), float(lr), 0, net.n_out

    def step(self, x, y):
        self.t += 1
        self.state, loss, self.last_grads = host_step(self.state, x, y, self.lr, self.t)
        return loss

    def l1_rows(self, x, y):
        return policy.host_l1_rows(policy.host_forward(self.state.net(), x), y)

    def _read(self, losses, errs):
        return np.concatenate([np.asarray(losses, np.float64).reshape(-1)] + [np.asarray(e, np.float64) for e in errs])

    def net(self):
        return self.state.net()


# ---- the device ------------------------------------------------------------------------------------------------------------------------

class DeviceTrainer(_Loop):
    def __init__(self, net, device="cuda", lr=0.002, keep_grads=False):
        """net: a PolicyNet, the initial weights (with BatchNorm its running statistics too); Adam starts from zero moments and count 0.
        keep_grads: every step also writes its gradients, which grads() returns; without it a gradient lives only in the register of
        the lane that applies it, and grads() raises.  .policy is a DevicePolicy on the packed image that every step rewrites, on the
        step's own stream: a reference to it stays current."""
        import torch
        self.torch, self.device, self.lr, self.t = torch, torch.device(device), float(lr), 0
        self.dims, self.eps, self.n_in, self.n_out = net.dims, net.eps, net.n_in, net.n_out
        up = lambda a: torch.from_numpy(np.array(a, dtype=_F)).to(self.device)      # noqa: E731
        state = TrainState.from_net(net)
        self.p, self.m, self.v = state.p.map(up), state.m.map(up), state.v.map(up)
        self.g = state.p.map(lambda a: torch.zeros(a.shape, dtype=torch.float32, device=self.device)) if keep_grads else None
        self.running_mean = [up(a) for a in state.running_mean] if net.batch_norm else None
        self.running_var = [up(a) for a in state.running_var] if net.batch_norm else None
        d = self.desc = _lib_policy_train.PolicyTrain()
        d.n_in, d.n_hidden, d.n_layers, d.n_out, d.batch_norm = net.dims
        d.eps = net.eps
        for mine, theirs in ((self.p, d.p), (self.m, d.m), (self.v, d.v)):
            self._point(theirs, mine)
        for l in range(net.n_layers if net.batch_norm else 0):
            d.running_mean[l], d.running_var[l] = self.running_mean[l].data_ptr(), self.running_var[l].data_ptr()
        if keep_grads:
            self.g_desc = _lib_policy_train.PolicyParams()
            self._point(self.g_desc, self.g)
        self.work = None
        self.tile = _lib_policy_train.lib().bmpc_policy_train_tile()
        self.policy = policy.DevicePolicy(net, self.device)      # on the image that every step rewrites (its .net stays the initial one)

    @staticmethod
    def _point(desc, params):
        for l, (w, b) in enumerate(zip(params.W, params.b)):
            desc.W[l], desc.b[l] = w.data_ptr(), b.data_ptr()
        for l in range(len(params.gamma or ())):
            desc.gamma[l], desc.beta[l] = params.gamma[l].data_ptr(), params.beta[l].data_ptr()

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _scratch(self, n):
        need = _lib_policy_train.lib().bmpc_policy_train_work_bytes(*self.dims, n)
        if need > 0 and (self.work is None or self.work.numel() * 4 < need):      # (a refused n is refused, and named, by the step itself)
            self.work = self.torch.empty(need // 4, dtype=self.torch.float32, device=self.device)
            self.desc.work, self.desc.work_bytes = self.work.data_ptr(), need
        elif self.work is None:
            self.desc.work, self.desc.work_bytes = None, 0

    def step(self, x, y, lr=None, out=None):
        """one training step on x (n, n_in), y (n, n_out), float64 device tensors used in place whatever their row strides (the pair that
        DeviceDatabase.batch returns).  lr: the learning rate from this step on.  Returns the loss, a float64 device scalar (`out`, a
        one-element float64 device tensor, where given); kernels on torch's current stream, no synchronisation."""
        if lr is not None:
            self.lr = float(lr)
        where = self.p.W[0].device
        s = _lib_policy_train.PolicyStep()
        s.x, s.x_stride = policy.device_rows(where, "x", x, self.n_in)
        s.n = n = x.shape[0]
        s.y, s.y_stride = policy.device_rows(where, "y", y, self.n_out, n)
        loss = self.torch.empty((), dtype=self.torch.float64, device=self.device) if out is None else out
        if loss.dtype != self.torch.float64 or loss.numel() != 1 or loss.device != where:
            raise ValueError("out: a one-element float64 tensor on %s is expected" % (self.device,))
        s.loss = loss.data_ptr()
        s.lr = self.lr
        s.bc1, s.bc2 = bias_corrections(self.t + 1)
        if self.g is not None:
            s.grads = C.addressof(self.g_desc)
        self._scratch(n)
        lib, stream, dp = _lib_policy_train.lib(), self._stream(), self.policy
        _lib.check(lib.bmpc_policy_train_step_device(C.byref(self.desc), C.byref(s), stream))
        self.t += 1
        # the packed image follows on the same stream: whoever holds .policy runs on the new weights, in stream order
        _lib.check(lib.bmpc_policy_pack_device(C.byref(self.desc), C.c_void_p(dp.packed.data_ptr()), dp.desc.packed_bytes, stream))
        return loss

    def grads(self):
        """the last step's gradients, a Params of device tensors (keep_grads=True)"""
        if self.g is None:
            raise ValueError("grads: the trainer was made without keep_grads=True")
        return self.g

    def l1_rows(self, x, y):
        return self.policy.l1_rows(x, y)

    def _read(self, losses, errs):
        torch = self.torch
        if not losses and not errs:
            return np.zeros(0)
        return torch.cat([v.reshape(-1) for v in list(losses) + list(errs)]).cpu().numpy()

    def state(self):
        """a TrainState on the host: parameters, moments, running statistics (synchronises)"""
        down = lambda t: t.cpu().numpy()      # noqa: E731
        bn = self.running_mean is not None
        return TrainState(self.p.map(down), self.m.map(down), self.v.map(down), [down(t) for t in self.running_mean] if bn else None,
                          [down(t) for t in self.running_var] if bn else None, self.eps)

    def net(self):
        """the current weights as a PolicyNet (synchronises)"""
        return self.state().net()

    def state_dict(self):
        """the reference's state_dict of the current weights, torch tensors on the trainer's device: GoalConditionedPolicyNet.load_state_dict
        takes it, and {"network": ...} of it is save_network's payload"""
        return {k: self.torch.from_numpy(np.array(v)).to(self.device) for k, v in state_dict_arrays(self.net(), self.t).items()}
