"""Cost of the Euclidean friction-cone projection (bmpc_cone_t, projection 1): the cone kernel against the diagonal one-wave kernel on
the same problems.

Shape: solo12_trot (four feet) and biped_walk (two feet), B = 4096, H = 20, harness form, 10 ADMM iterations, cold start, fp64, one
wave per SIMD forced for the diagonal leg (the cone kernel has no two-waves build, so like is compared with like) and its step
certificate off (the cone kernel tests every step).  Three legs: the diagonal kernel (the reference's projection, the batch's scalar mu),
the cone kernel with one set of coefficients shared by the batch (stride 0) and with coefficients per problem; every coefficient is the
batch's scalar mu, so the three legs solve the same problems and differ only where a force leaves the cone -- another projection there,
so the FISTA iteration counts may differ and the times are also given per 1000 FISTA iterations.  One JSON line:

  events     per foot count the legs interleaved in one process, median, min and max of --runs launches each (torch events)
  scratch    the cone unit's private-segment bytes per lane, per foot count (the largest over its kernels)

The GPU step runs in a child process under a time limit.

    python tools/cone_bench.py [--runs 7] [--warmup 2] [--B 4096] [--iters 10] [--mu MU]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 300
CONFIGS = ("solo12_trot", "biped_walk")


def legs(config, B, iters, mu):
    from bunmpc_amd import batch as bb
    from bunmpc_amd import problems
    b = problems.make_batch(config, B)
    mu = b.mu if mu is None else mu
    shared, per_problem = np.full((1, b.H, b.E), mu), np.full((B, b.H, b.E), mu)
    return b, mu, {"diagonal": bb.DeviceBatch(b, num_iters=iters, mu=mu),
                   "cone_shared": bb.DeviceBatch(b, num_iters=iters, cone=dict(projection="euclidean", mu=shared)),
                   "cone_per_problem": bb.DeviceBatch(b, num_iters=iters, cone=dict(projection="euclidean", mu=per_problem))}


def measure(args):
    from bunmpc_amd import _lib
    lib = _lib.lib()
    out = {config: measure_config(args, config) for config in CONFIGS}
    out["scratch_bytes_per_lane"] = {"n_eff_4": lib.bmpc_biconvex_cone_kernel_scratch_bytes(4), "n_eff_2": lib.bmpc_biconvex_cone_kernel_scratch_bytes(2),
                                     "diagonal_n_eff_4": lib.bmpc_biconvex_kernel_scratch_bytes(4, 0), "diagonal_n_eff_2": lib.bmpc_biconvex_kernel_scratch_bytes(2, 0)}
    return out


def measure_config(args, config):
    import torch
    from bunmpc_amd import _lib
    lib = _lib.lib()
    lib.bmpc_set_two_waves_per_simd(0)
    lib.bmpc_set_latency_mapping_max_batch(0)
    lib.bmpc_set_certified_steps(0)
    b, mu, dev = legs(config, args.B, args.iters, args.mu)
    out = {"config": config, "n_eff": b.E, "B": args.B, "H": b.H, "admm_iters": args.iters, "runs": args.runs, "mu": mu}
    ms = {k: [] for k in dev}
    for r in range(args.warmup + args.runs):
        for k, d in dev.items():      # interleaved
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            d.solve()
            e1.record()
            torch.cuda.synchronize()
            if r == 0:
                out[k] = {"kernel": lib.bmpc_biconvex_last_kernel_name().decode(), "lanes_per_problem": lib.bmpc_biconvex_last_lanes_per_problem(),
                          "waves_per_simd": lib.bmpc_biconvex_last_waves_per_simd()}
            if r >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
    for k, d in dev.items():
        st = d.results()["stats"]
        fista = float(st[:, 1:3].sum(axis=1).mean())
        out[k].update(ms_median=float(np.median(ms[k])), ms_min=float(np.min(ms[k])), ms_max=float(np.max(ms[k])), fista_iters_per_solve=fista,
                      retries_per_solve=float(st[:, 3:5].sum(axis=1).mean()), ms_per_1000_fista_iters=1000.0 * float(np.median(ms[k])) / fista,
                      diverged=int((st[:, 5] != 0).sum()))
    for k in ("cone_shared", "cone_per_problem"):
        out["ratio_%s_over_diagonal" % k] = out[k]["ms_median"] / out["diagonal"]["ms_median"]
        out["ratio_%s_per_fista_iteration" % k] = out[k]["ms_per_1000_fista_iters"] / out["diagonal"]["ms_per_1000_fista_iters"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--mu", type=float, default=None, help="the friction coefficient of every leg (default: the batch's own)")
    ap.add_argument("--leg", choices=["measure"], help="(internal) run the measurement in this process and print its JSON")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.runs < 5:
        ap.error("--runs: at least five runs of each leg")
    if args.leg:
        print(json.dumps(measure(args)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--leg", "measure", "--runs", str(args.runs), "--warmup", str(args.warmup), "--B", str(args.B),
          "--iters", str(args.iters)] + ([] if args.mu is None else ["--mu", str(args.mu)])
    out = {"workload": "cone kernel (Euclidean friction-cone projection) against the diagonal harness-form kernel, one wave per SIMD", "date": time.strftime("%Y-%m-%d")}
    try:
        p = subprocess.run(me, cwd=ROOT, capture_output=True, text=True, timeout=TIMEOUT_S)
        if p.returncode != 0:
            out["events"] = {"error": "exit status %d" % p.returncode, "stderr_tail": p.stderr[-800:]}
        else:
            out["events"] = json.loads(p.stdout.strip().splitlines()[-1])
    except subprocess.TimeoutExpired:
        out["events"] = {"error": "timed out after %d s" % TIMEOUT_S}
    print(json.dumps(out))
    if "error" in out["events"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
