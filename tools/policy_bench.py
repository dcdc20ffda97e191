"""Time per call of the policy network's forward pass on the device (bunmpc_amd/policy.py::DevicePolicy.forward) against what a user
has without it: the same nn.Sequential evaluated by torch in fp32 on the same GPU.

Net: (55, 256, 4 hidden layers, 12), the reference's default width, weights from a fixed seed.  Input: x (n, 55) float64 on the device,
as DeviceDatabase.batch returns it.  Legs at every n of --n, interleaved in one process (every sample of a leg follows a sample of the
other):

  device   DevicePolicy.forward(x): one kernel, action (n, 12) float64                   events around `calls` back-to-back calls
  torch    net(x.float()) under no_grad: the cast and nine kernels, action float32       events around `calls` back-to-back calls

calls is --calls, scaled down at large n so that a sample stays a few milliseconds at least.  Per leg the median, minimum and maximum of
--runs samples; for the device leg the multiply-adds of the four products, 2 n sum(K N) FLOP, over the median time, and that rate as a
share of the fp32 matrix peak (--peak, 157.3 TFLOP/s on the MI355X) -- a whole-call rate: launch, prologue and epilogue included.  The
two results are compared once (the largest difference over the largest output), so that both legs are seen to compute the same net.
One JSON line.

    python tools/policy_bench.py [--runs 15] [--warmup 3] [--calls 200] [--n 1 256 4096 65536]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DIMS = (55, 256, 4, 12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--n", type=int, nargs="+", default=[1, 256, 4096, 65536])
    ap.add_argument("--peak", type=float, default=157.3e12, help="fp32 matrix FLOP per second")
    args = ap.parse_args()
    import torch
    from bunmpc_amd import policy
    dev = "cuda:0"
    n_in, hidden, layers, n_out = DIMS
    rng = np.random.default_rng(256)
    K, N = [n_in] + [hidden] * layers, [hidden] * layers + [n_out]
    net = policy.PolicyNet.from_arrays([rng.normal(size=(n, k)) * np.sqrt(2.0 / k) for n, k in zip(N, K)], [rng.normal(size=n) * 0.2 for n in N])
    dp = policy.DevicePolicy(net, dev)
    mods = []
    for l in range(layers + 1):
        lin = torch.nn.Linear(K[l], N[l])
        lin.load_state_dict(dict(weight=torch.from_numpy(net.W[l]), bias=torch.from_numpy(net.b[l])))
        mods += [lin] + ([torch.nn.ReLU()] if l < layers else [])
    seq = torch.nn.Sequential(*mods).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    flop_per_row = 2 * sum(k * n for k, n in zip(K, N))
    out = {}
    with torch.no_grad():
        for n in args.n:
            x = torch.randn((n, n_in), dtype=torch.float64, device=dev, generator=g)
            calls = max(10, min(args.calls, args.calls * 4096 // max(n, 1)))
            legs = {"device": lambda: dp.forward(x), "torch": lambda: seq(x.float())}
            a, b = legs["device"]().cpu().numpy(), legs["torch"]().double().cpu().numpy()
            samples = {k: [] for k in legs}
            for r in range(args.warmup + args.runs):
                for k, call in legs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        call()
                    e1.record()
                    e1.synchronize()
                    if r >= args.warmup:
                        samples[k].append(1e3 * e0.elapsed_time(e1) / calls)
            res = {k: dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v))) for k, v in samples.items()}
            rate = n * flop_per_row / (1e-6 * res["device"]["median_us"])
            res["device"].update(flop=n * flop_per_row, TFLOP_per_s=rate / 1e12, share_of_fp32_matrix_peak=rate / args.peak)
            res.update(calls=calls, torch_over_device=res["torch"]["median_us"] / res["device"]["median_us"],
                       max_difference_over_max_output=float(np.abs(a - b).max() / np.abs(a).max()))
            out[str(n)] = res
    print(json.dumps(dict(net=DIMS, runs=args.runs, tile=dp.tile, us_per_call=out)))


if __name__ == "__main__":
    main()
