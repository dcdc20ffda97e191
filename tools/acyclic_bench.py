"""Acyclic motions on the device, timed on the synthetic hop table of the tests (tests/acyclic_np.py) at B = 4096:

  plan      bmpc_acyclic_plan_batch_device against bmpc_wb_plan_batch_device (the cyclic harness' plan call, Solo12 trot) on the same B:
            device events around `reps` calls after a warm-up, median per call;
  optimize  BatchedAcyclicMpc.optimize (plan -> centroidal ADMM + IK-DDP -> 1 kHz rows, synchronised) against B calls of
            SoloAcyclicGen.optimize through the single-problem handle: the handle is timed on `sample` problems of the batch (host
            clock, every call ends in copies that synchronise) and scaled to B.

Needs a GPU: there is no fallback.  Prints one JSON line; --out also writes it to a file.

    python tools/acyclic_bench.py [--B 4096] [--reps 20] [--sample 32] [--dyn-iters 50] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch_inputs(B, seed=7):
    """B perturbed jump states at motion times spread over the table and beyond it"""
    from tests import acyclic_np as twin
    rng = np.random.default_rng(seed)
    x = np.tile(twin.states()[0], (B, 1))
    x[:, 0:3] += rng.normal(0, 0.01, (B, 3))
    quat = x[:, 3:7] + rng.normal(0, 0.02, (B, 4))
    x[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    x[:, 7:19] += rng.normal(0, 0.05, (B, 12))
    x[:, 19:] = rng.normal(0, 0.1, (B, 18))
    return x, np.round(rng.uniform(0.0, 1.0, B), 2), np.zeros(B)


def device_ms(fn, warmup, reps):
    """median time of fn() in ms between device events"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sample", type=int, default=32)
    ap.add_argument("--dyn-iters", type=int, default=50)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("acyclic_bench needs a GPU")
    from bunmpc_amd import problems, urdf_model
    from bunmpc_amd.acyclic_batch import BatchedAcyclicMpc, DeviceAcyclicPlan
    from bunmpc_amd.acyclic_gen import SoloAcyclicGen
    from bunmpc_amd.mpc_batch import BatchedMpc
    from bunmpc_amd.plan_batch import DeviceWbPlan
    from tests import acyclic_np as twin
    model = urdf_model.RobotModel.from_json(open(os.path.join(ROOT, "bunmpc_amd", "robots", "solo12.json")).read())
    B = args.B
    x, t, t0 = batch_inputs(B)
    mpc = BatchedAcyclicMpc(model, twin.hop_plan(), dyn_iters=args.dyn_iters)
    res = dict(tool="acyclic_bench", B=B, H=mpc.H, dyn_iters=args.dyn_iters, reps=args.reps, device=torch.cuda.get_device_name(0))
    # ---- the plan calls
    acy = DeviceAcyclicPlan(mpc.table, B, x, t, t0)
    cyc = BatchedMpc(model)
    wbp = DeviceWbPlan(cyc.dm, cyc.gait, cyc.offsets_xy, cyc.wb.feet, cyc.ik, x, t, np.tile([0.2, 0.0, 0.0], (B, 1)), cyc.H, cyc.T)
    for name, plan in (("acyclic_plan_ms", acy), ("wb_plan_ms", wbp)):
        res[name] = dict(zip(("median", "min", "max"), device_ms(plan.build, 5, args.reps)))
    res["wb_plan_shape"] = dict(H=cyc.H, T=cyc.T)
    # ---- optimize: the batch (synchronised: a host clock around work that ends in a device synchronise)
    times = []
    for _ in range(2 + max(args.reps // 4, 3)):
        torch.cuda.synchronize()
        c = time.perf_counter()
        out = mpc.optimize(x, t, t0)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - c))
    res["batched_optimize_ms"] = dict(median=statistics.median(times[2:]), min=min(times[2:]), max=max(times[2:]), first=times[0])
    r = out["solver"].results()
    res["ik_iters"] = dict(mean=float(r["ik_iters"].mean()), max=int(r["ik_iters"].max()), unconverged=int((r["ik_status"] != 0).sum()))
    # ---- optimize: the handle, one call per problem, on a bounded sample
    gen = SoloAcyclicGen(model, model)
    gen.dyn_iters = args.dyn_iters
    idx = np.linspace(0, B - 1, args.sample).astype(int)
    per = []
    for k, b in enumerate([idx[0]] + list(idx)):      # (the first call warms the handle up and is not counted)
        c = time.perf_counter()
        gen.update_motion_params(twin.hop_plan(), x[b, :19].copy(), float(t0[b]))
        gen.optimize(x[b, :19].copy(), x[b, 19:].copy(), float(t[b]))
        if k:
            per.append(1e3 * (time.perf_counter() - c))
    res["handle_call_ms"] = dict(median=statistics.median(per), min=min(per), max=max(per), sample=len(per))
    res["handle_scaled_to_B_ms"] = statistics.mean(per) * B
    res["speedup_optimize"] = res["handle_scaled_to_B_ms"] / res["batched_optimize_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
