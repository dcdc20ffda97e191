"""Timings of the centroidal solve for bipeds (n_eff = 2; problems.make_batch("biped_walk"): walk / hop mix, H = 20).  One JSON line:

  batch_10      B = 4096, 10 ADMM iterations (the default dispatch: 32-lane segments)
  batch_100     B = 4096, 100 ADMM iterations (the work-stealing kernel)
  latency       batch-1 BiconvexMP(m, H, 2).optimize(x, 10) p50 (the one-problem-per-wave kernel)
  quad_10       the quadruped headline shape for comparison (solo12_trot, B = 4096, H = 20, 10 ADMM iterations)

Per launch: solves/s, ms per launch (mean of torch events), the kernel name and waves per SIMD it reports, the summed FISTA iterations
per solve (force + motion, mean over the batch) and ms per 1000 of them.  Every leg runs in a child process of its own under a time
limit; the first leg that fails ends the run.

    python tools/biped_bench.py [--steps 20] [--warmup 3] [--reps 200]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"batch_10": ("biped_walk", 4096, 10), "batch_100": ("biped_walk", 4096, 100), "latency": ("biped_walk", 1, 10),
        "quad_10": ("solo12_trot", 4096, 10)}
TIMEOUT_S = {"batch_10": 180, "batch_100": 240, "latency": 180, "quad_10": 180}


def batch_leg(config, B, iters, steps, warmup):
    import torch
    from bunmpc_amd import _lib
    from bunmpc_amd import batch as bb
    from bunmpc_amd import problems
    b = problems.make_batch(config, B)
    db = bb.DeviceBatch(b, num_iters=iters)
    for _ in range(warmup):
        db.solve()
    torch.cuda.synchronize()
    lib = _lib.lib()
    kernel, wpe, lpp = lib.bmpc_biconvex_last_kernel_name().decode(), lib.bmpc_biconvex_last_waves_per_simd(), lib.bmpc_biconvex_last_lanes_per_problem()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for s in range(steps):
        ev[s][0].record()
        db.solve()
        ev[s][1].record()
    torch.cuda.synchronize()
    ms = float(np.mean([a.elapsed_time(c) for a, c in ev]))
    st = db.results()["stats"]
    fista = float(st[:, 1:3].sum(axis=1).mean())
    return {"config": config, "n_eff": b.E, "B": B, "H": b.H, "admm_iters": iters, "ms_per_launch": ms, "solves_per_s": B / (ms * 1e-3),
            "kernel": kernel, "waves_per_simd": wpe, "lanes_per_problem": lpp, "fista_iters_per_solve": fista,
            "ms_per_1000_fista_iters": 1000.0 * ms / fista, "diverged": int((st[:, 5] != 0).sum()), "steps": steps}


def latency_leg(config, iters, reps, warm):
    from bunmpc_amd import _lib
    from bunmpc_amd import problems
    from bunmpc_amd.biconvex_mpc_cpp import BiconvexMP
    b = problems.make_batch(config, 1)
    mp = BiconvexMP(b.m, b.H, b.E)
    mp.set_rho(b.rho)
    mp.set_friction_coefficient(b.mu)
    X0, F0, P0 = b.warm_start()
    ts = []
    for _ in range(reps + warm):
        for i in range(b.H):
            mp.set_contact_plan(b.cnt_plan[0, i], b.dt[0, i])
        mp.create_bound_constraints(b.bounds[0], 15.0, 15.0, 15.0)
        mp.create_cost_X(b.W_X[0], b.W_X_ter[0], b.X_ter[0], b.X_nom[0])
        mp.create_cost_F(b.W_F[0])
        mp.set_warm_start_vars(X0[0], F0[0], P0[0])
        mp.set_step_constants(2.25e6, 506.25)
        t0 = time.perf_counter()
        mp.optimize(b.x_init[0], iters)
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts[warm:]) * 1e3
    lib = _lib.lib()
    st = mp.last_stats()
    return {"config": config, "n_eff": b.E, "H": b.H, "admm_iters": iters, "p50_ms": float(np.median(ts)), "p90_ms": float(np.quantile(ts, 0.9)),
            "reps": reps, "warmups": warm, "kernel": lib.bmpc_biconvex_last_kernel_name().decode(),
            "waves_per_simd": lib.bmpc_biconvex_last_waves_per_simd(), "fista_iters_per_solve": int(st[1] + st[2])}


def run_leg(name, args):
    config, B, iters = LEGS[name]
    if name == "latency":
        return latency_leg(config, iters, args.reps, 20)
    return batch_leg(config, B, iters, args.steps, args.warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--leg", choices=sorted(LEGS), help="(internal) run one leg in this process and print its JSON")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.leg:
        print(json.dumps(run_leg(args.leg, args)))
        return
    out = {"workload": "biped_walk centroidal solve (n_eff = 2), BiconvexMP.optimize semantics", "date": time.strftime("%Y-%m-%d")}
    for name in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--reps", str(args.reps)]
        try:
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=TIMEOUT_S[name])
        except subprocess.TimeoutExpired:
            out[name] = {"error": "timed out after %d s" % TIMEOUT_S[name]}
            break
        if p.returncode != 0:
            out[name] = {"error": "exit status %d" % p.returncode, "stderr_tail": p.stderr[-800:]}
            break
        out[name] = json.loads(p.stdout.strip().splitlines()[-1])
    b10, q10 = out.get("batch_10", {}), out.get("quad_10", {})
    if "ms_per_1000_fista_iters" in b10 and "ms_per_1000_fista_iters" in q10:
        out["fista_iter_time_ratio_biped_over_quad"] = b10["ms_per_1000_fista_iters"] / q10["ms_per_1000_fista_iters"]
    print(json.dumps(out))
    if any("error" in v for v in out.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
