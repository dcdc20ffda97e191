"""Time per training step of the policy network on the device (bunmpc_amd/policy_train.py::DeviceTrainer.step) against what a user has
without it: the same nn.Sequential trained by eager torch in fp32 on the same GPU with the reference's loop body (zero_grad, .float(),
forward in train() mode, nn.L1Loss, backward, torch.optim.Adam.step).

Nets: (55, 256, 4 hidden layers, 12) without and with BatchNorm1d and (91, 512, 3, 12), weights from a fixed seed.  Batch: x (256, in),
y (256, 12) float64 on the device, as DeviceDatabase.batch returns them.  Legs, interleaved in one process (every sample of a leg follows
a sample of the other):

  device   DeviceTrainer.step(x, y): 3 n_layers + 4 kernels and the packed image's       events around `calls` back-to-back steps
  torch    the loop body above on the same rows                                          events around `calls` back-to-back steps

Per leg the median, minimum and maximum of --runs samples.  Both legs start from the same weights and their losses after the timed steps
are printed side by side, so that both are seen to train the same net.

Then one epoch of DeviceTrainer.fit on a DeviceDatabase of --rows rows (90 % training rows in batches of 256, then the validation loss
over the rest) against the reference's loop over the same rows held on the device: torch.utils.data.DataLoader(shuffle, drop_last) over
a Dataset whose __getitem__ returns one row, the loop body above, then the eval() pass over a second DataLoader.  Wall-clock time around a
synchronised epoch, --epoch-runs samples per leg after one warm-up epoch.  One JSON line.

    python tools/policy_train_bench.py [--runs 15] [--warmup 3] [--calls 100] [--rows 200000] [--epoch-runs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NETS = [(55, 256, 4, 12, False), (55, 256, 4, 12, True), (91, 512, 3, 12, False)]
N, LR = 256, 0.002


def drawn_net(dims, seed=256):
    from bunmpc_amd import policy
    n_in, hidden, layers, n_out, bn = dims
    rng = np.random.default_rng(seed)
    K, Nw = [n_in] + [hidden] * layers, [hidden] * layers + [n_out]
    norm = [(np.ones(hidden), np.zeros(hidden), np.zeros(hidden), np.ones(hidden)) for _ in range(layers)] if bn else None
    return policy.PolicyNet.from_arrays([rng.normal(size=(n, k)) * np.sqrt(2.0 / k) for n, k in zip(Nw, K)], [rng.normal(size=n) * 0.2 for n in Nw], norm)


def torch_module(net, dev):
    """the reference's nn.Sequential with `net`'s weights"""
    import torch
    from bunmpc_amd import policy_train
    mods = []
    for l in range(net.n_layers + 1):
        mods.append(torch.nn.Linear(*net.W[l].shape[::-1]))
        if l < net.n_layers:
            mods += ([torch.nn.BatchNorm1d(net.n_hidden, eps=net.eps)] if net.batch_norm else []) + [torch.nn.ReLU()]
    module = torch.nn.Module()
    module.net = torch.nn.Sequential(*mods)
    module.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in policy_train.state_dict_arrays(net).items()})
    return module.to(dev)


def torch_step(module, opt, criterion, x, y):
    opt.zero_grad()
    loss = criterion(module.net(x.float()), y.float())
    loss.backward()
    opt.step()
    return loss


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def step_times(args, dev):
    import torch
    from bunmpc_amd import policy_train
    out = {}
    for dims in NETS:
        net = drawn_net(dims)
        trainer = policy_train.DeviceTrainer(net, dev, lr=LR)
        module = torch_module(net, dev).train()
        opt, criterion = torch.optim.Adam(module.parameters(), lr=LR), torch.nn.L1Loss()
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn((N, dims[0]), dtype=torch.float64, device=dev, generator=g)
        y = torch.randn((N, dims[3]), dtype=torch.float64, device=dev, generator=g)
        legs = {"device": lambda: trainer.step(x, y), "torch": lambda: torch_step(module, opt, criterion, x, y)}
        samples, last = {k: [] for k in legs}, {}
        for r in range(args.warmup + args.runs):
            for k, call in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    last[k] = call()
                e1.record()
                e1.synchronize()
                if r >= args.warmup:
                    samples[k].append(1e3 * e0.elapsed_time(e1) / args.calls)
        res = {k: stats(v) for k, v in samples.items()}
        res.update(launches_per_step=3 * dims[2] + 5, torch_over_device=res["torch"]["median"] / res["device"]["median"],
                   loss_after=dict(device=float(last["device"]), torch=float(last["torch"].detach())), steps_each=(args.warmup + args.runs) * args.calls)
        out["%d-%d-%d-%d%s" % (dims[:4] + ("-bn" if dims[4] else "",))] = res
    return out


def epoch_times(args, dev):
    import torch
    from bunmpc_amd import policy_train
    from bunmpc_amd.dataset_device import DeviceDatabase
    g = torch.Generator(device=dev).manual_seed(1)
    rows = args.rows
    draw = lambda w: torch.randn((rows, w), dtype=torch.float64, device=dev, generator=g)      # noqa: E731
    db = DeviceDatabase(rows, goal_horizon=1, device=dev, max_problems=max(rows, 1 << 18))
    db.append(states=draw(43), actions=draw(12), vc_goals=draw(5), cc_goals=draw(12))
    db.calc_input_mean_std()
    net = drawn_net(NETS[0])
    trainer = policy_train.DeviceTrainer(net, dev, lr=LR)
    module = torch_module(net, dev)
    opt, criterion = torch.optim.Adam(module.parameters(), lr=LR), torch.nn.L1Loss()
    xs, ys = db.batch(torch.arange(rows, device=dev))      # the same normalised rows, held on the device

    class Rows(torch.utils.data.Dataset):
        def __len__(self):
            return rows

        def __getitem__(self, i):
            return xs[i], ys[i]

    n_train = int(0.9 * rows)
    train_data, test_data = torch.utils.data.random_split(Rows(), [n_train, rows - n_train])
    train_loader = torch.utils.data.DataLoader(train_data, N, shuffle=True, drop_last=True)
    test_loader = torch.utils.data.DataLoader(test_data, N, shuffle=True, drop_last=True)

    def torch_epoch():
        module.train()
        train, valid = [], []
        for x, y in train_loader:
            train.append(torch_step(module, opt, criterion, x, y).item())
        module.eval()
        for x, y in test_loader:
            valid.append(criterion(module.net(x.float()), y.float()).item())
        return float(np.mean(train)), float(np.mean(valid))

    legs = {"device": lambda: trainer.fit(db, n_epoch=1, batch_size=N, n_train_frac=0.9, seed=0)[0], "torch": torch_epoch}
    samples, last = {k: [] for k in legs}, {}
    for r in range(1 + args.epoch_runs):
        for k, call in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = call()
            torch.cuda.synchronize()
            if r >= 1:
                samples[k].append(time.perf_counter() - t0)
    res = {k: stats(v) for k, v in samples.items()}
    res.update(rows=rows, steps_per_epoch=n_train // N, torch_over_device=res["torch"]["median"] / res["device"]["median"],
               losses_after=dict(device=last["device"], torch=last["torch"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--epoch-runs", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda:0"
    out = dict(n=N, runs=args.runs, calls=args.calls, us_per_step=step_times(args, dev))
    if args.rows:
        out["s_per_epoch"] = epoch_times(args, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
