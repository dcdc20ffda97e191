"""Record tests/golden/policy/train_ref.npz: training steps of the REFERENCE's own policy network under the reference's loop.

Run by hand, on a machine that has the reference beside this repository, with torch on the CPU:

    python tests/golden/make_golden_policy_train.py <path of iterative_supervised_learning> [--out tests/golden/policy/train_ref.npz]

It loads examples/iterative_algorithm/networks.py from its place, builds GoalConditionedPolicyNet as the trainers do and runs the loop of
behavioral_cloning_train.py:123-149 on it: train() mode, nn.L1Loss(), loss.backward(), torch.optim.Adam(lr = 0.002).  Its initialisation
leaves every bias zero, so the biases are redrawn, and BatchNorm1d's affine terms and running statistics are moved away from (1, 0, 0, 1).
Only arrays go into the file; no test reads the reference.

A "parameter vector" below is one flat array: every parameter in the order of parameters() -- W<l>, b<l>, then gamma<l>, beta<l> with
BatchNorm, per layer -- each row-major, concatenated.  Per net `n<i>_`: dims (in, hidden, hidden layers, out, batch_norm), eps, lr, `init`
the parameter vector before the first step, init_rm, init_rv (hidden layers, hidden) the running statistics.  Per step `n<i>_s<k>_`,
k = 0, 1, 2 consecutive from there (Adam's count t = k + 1; the state before step k + 1 is the state after step k):
    x (40, in), y (40, out) float32     the batch as the loop's .float() leaves it (drawn in float64)
    loss, pred, g                       float32: the loss, the predictions, the gradients' parameter vector
    p, m, v, rm, rv                     float32: parameters, exp_avg, exp_avg_sq (parameter vectors) and running statistics AFTER the step
    bmean, bvar                         float32 (hidden layers, hidden): the batch's mean and biased variance of the values entering each
                                        BatchNorm1d
    d, dpred, dloss, dbmean, dbvar, drm, drv
                                        the same step taken by a .double() copy of the fp32 state BEFORE this step (float32 input rows widened):
                                        the float64 gradient is float64(g) + float64(d) and the float64 prediction float64(pred) +
                                        float64(dpred) -- the difference is stored, as float32, because that keeps 24 bits of the
                                        difference at half the bytes -- the others are float64.  The file has to stay under 1 MiB
                                        (tests/test_policy_train_cpu.py asserts it), and the parameter vectors are what fills it.
    c_loss                              float64: the same three steps taken consecutively by a .double() copy of the initial state (its
                                        weights drift from the fp32 run's by Adam's steps, so only the loss is kept)
and for net 0 `n0_s1000_`: one more step after the optimizer's state was set by hand to step = 999 with drawn exp_avg, exp_avg_sq (stored
before the step as m0, v0; the parameters and running statistics before it are those after step 2), so that both bias corrections are far
from those of the first steps.

The generator asserts, in float64 and for every recorded step, that every value entering a ReLU and every p - y is at least 1e-4 away
from 0, and walks seeds until that holds: no mask and no sign can then differ between the precisions."""
import argparse
import copy
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NETS = [(23, 24, 2, 12, True), (23, 48, 2, 36, False), (55, 40, 3, 12, True)]
ROWS, LR, MARGIN = 40, 0.002, 1e-4


def names(net):
    """the order of parameters(): W<l>, b<l>, and gamma<l>, beta<l> after a hidden layer's with BatchNorm"""
    out, l = [], 0
    for m in net.net:
        if isinstance(m, torch.nn.Linear):
            out += ["W%d" % l, "b%d" % l]
            l += 1
        elif isinstance(m, torch.nn.BatchNorm1d):
            out += ["gamma%d" % (l - 1), "beta%d" % (l - 1)]
    return out


def norms(net):
    return [m for m in net.net if isinstance(m, torch.nn.BatchNorm1d)]


def one_step(net, opt, x, y):
    """the loop's body; returns (loss, pred, grads, [inputs of BatchNorm1d], min |ReLU input|)"""
    seen, relu_in = [], []
    hooks = [m.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].detach().clone())) for m in norms(net)]
    hooks += [m.register_forward_hook(lambda mod, inp, out: relu_in.append(inp[0].detach().abs().min().item())) for m in net.net if isinstance(m, torch.nn.ReLU)]
    net.train()
    opt.zero_grad()
    pred = net(x)
    loss = torch.nn.L1Loss()(pred, y)
    loss.backward()
    grads = [p.grad.detach().clone() for p in net.parameters()]
    opt.step()
    for h in hooks:
        h.remove()
    return loss.detach(), pred.detach(), grads, seen, min(relu_in)


def record(networks, dims, seed):
    """the arrays of one net, or None where a margin is missed"""
    n_in, hidden, layers, n_out, bn = dims
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    net = networks.GoalConditionedPolicyNet(n_in, n_out, num_hidden_layer=layers, hidden_dim=hidden, batch_norm=bn)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0.0, 0.2)
            elif isinstance(m, torch.nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.3)
                m.running_mean.normal_(0.0, 0.5)
                m.running_var.uniform_(0.3, 2.5)
    q = names(net)
    out = {"dims": np.array([n_in, hidden, layers, n_out, int(bn)]), "eps": np.array(norms(net)[0].eps if bn else 1e-5), "lr": np.array(LR)}

    def put(prefix, values):
        values = list(values)      # one flat array per kind (an entry of the file costs more than a small array holds)
        assert len(values) == len(q)
        out[prefix[:-1]] = np.concatenate([v.detach().numpy().reshape(-1) for v in values])

    def put_running(prefix, a, b, net_):
        if bn:
            out[prefix + a] = np.stack([m.running_mean.numpy() for m in norms(net_)])
            out[prefix + b] = np.stack([m.running_var.numpy() for m in norms(net_)])

    put("init_", net.parameters())
    put_running("init_", "rm", "rv", net)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    chain64 = copy.deepcopy(net).double()
    opt64 = torch.optim.Adam(chain64.parameters(), lr=LR)

    def step(k):
        s = "s%d_" % k
        x, y = rng.normal(size=(ROWS, n_in)), rng.normal(size=(ROWS, n_out))
        x32, y32 = torch.from_numpy(x).float(), torch.from_numpy(y).float()
        twin = copy.deepcopy(net).double()      # the fp32 state before this step, in float64
        loss64, pred64, g64, seen64, margin = one_step(twin, torch.optim.Adam(twin.parameters(), lr=LR), x32.double(), y32.double())
        if margin < MARGIN or (pred64 - y32.double()).abs().min().item() < MARGIN:
            return False
        loss, pred, g, seen, _ = one_step(net, opt, x32, y32)
        out[s + "x"], out[s + "y"], out[s + "loss"], out[s + "pred"] = x32.numpy(), y32.numpy(), loss.numpy(), pred.numpy()
        out[s + "dloss"], out[s + "dpred"] = loss64.numpy(), (pred64 - pred.double()).float().numpy()
        put(s + "g_", g)
        put(s + "d_", [(b - a.double()).float() for a, b in zip(g, g64)])
        put(s + "p_", net.parameters())
        put(s + "m_", [opt.state[p]["exp_avg"] for p in net.parameters()])
        put(s + "v_", [opt.state[p]["exp_avg_sq"] for p in net.parameters()])
        put_running(s, "rm", "rv", net)
        put_running(s, "drm", "drv", twin)
        if bn:
            out[s + "bmean"], out[s + "bvar"] = np.stack([a.mean(0).numpy() for a in seen]), np.stack([a.var(0, unbiased=False).numpy() for a in seen])
            out[s + "dbmean"], out[s + "dbvar"] = np.stack([a.mean(0).numpy() for a in seen64]), np.stack([a.var(0, unbiased=False).numpy() for a in seen64])
        if k < 3:
            c_loss, c_pred, _, _, c_margin = one_step(chain64, opt64, x32.double(), y32.double())
            if c_margin < MARGIN or (c_pred - y32.double()).abs().min().item() < MARGIN:
                return False
            out[s + "c_loss"] = c_loss.numpy()
        return True

    for k in range(3):
        if not step(k):
            return None
    if dims == NETS[0]:
        with torch.no_grad():
            for p in net.parameters():
                st = opt.state[p]
                st["step"].fill_(999.0)
                st["exp_avg"].copy_(torch.from_numpy(rng.normal(size=tuple(p.shape)) * 1e-3))
                st["exp_avg_sq"].copy_(torch.from_numpy((rng.normal(size=tuple(p.shape)) * 1e-3) ** 2 + 1e-9))
        put("s1000_m0_", [opt.state[p]["exp_avg"] for p in net.parameters()])
        put("s1000_v0_", [opt.state[p]["exp_avg_sq"] for p in net.parameters()])
        if not step(1000):
            return None
        assert all(int(opt.state[p]["step"].item()) == 1000 for p in net.parameters())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("isl")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "policy", "train_ref.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("networks", os.path.join(args.isl, "examples", "iterative_algorithm", "networks.py"))
    networks = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(networks)
    torch.set_num_threads(1)
    out = {}
    for i, dims in enumerate(NETS):
        seed = 20240901 + 1000 * i
        while (arrays := record(networks, dims, seed)) is None:
            seed += 1
        print("net %d %s: seed %d" % (i, dims, seed))
        out.update({"n%d_%s" % (i, k): v for k, v in arrays.items()})
        out["n%d_seed" % i] = np.array(seed)
    out["n_nets"] = np.asarray(len(NETS))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print("%d nets -> %s (%d bytes)" % (len(NETS), args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
