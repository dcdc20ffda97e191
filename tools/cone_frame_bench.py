"""Cost of friction cones about per-contact surface normals (bmpc_contact_frame_t): the kernel about normals against the cone kernel.

Shape: solo12_trot (four feet) and biped_walk (two feet), B = 4096, H = 20, harness form, 10 ADMM iterations, cold start, fp64, one
wave per SIMD (both kernel families have that build only), one friction coefficient for every foot (--mu, default 0.3).  Three legs:

  cone            the cone kernel (world z)
  frames_world_z  the kernel about normals with (0, 0, 1) everywhere, shared by the batch: the cone leg's values and iteration counts,
                  so the ratio is the cost of the added instructions alone
  frames_slope    the kernel about normals on a plane tilted by --roll / --pitch degrees (default 10 / 25: beyond atan(0.3) = 16.7
                  degrees, so the cones bind), normals per problem: another problem, so the FISTA iteration counts differ and the times
                  are also given per 1000 FISTA iterations

One JSON line:

  events     per foot count the legs interleaved in one process, median, min and max of --runs launches each (torch events)
  scratch    the two units' private-segment bytes per lane, per foot count (the largest over their kernels)

The GPU step runs in a child process under a time limit.

    python tools/cone_frame_bench.py [--runs 9] [--warmup 2] [--B 4096] [--iters 10] [--mu 0.3] [--roll 10] [--pitch 25]
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


def legs(config, B, iters, mu, roll, pitch):
    from bunmpc_amd import batch as bb
    from bunmpc_amd import problems
    b = problems.make_batch(config, B)
    world_z = problems.plane_normals(1, b.H, b.E, 0.0, 0.0)
    slope = problems.plane_normals(B, b.H, b.E, np.deg2rad(roll), np.deg2rad(pitch))
    return b, {"cone": bb.DeviceBatch(b, num_iters=iters, mu=mu, cone=dict(projection="euclidean")),
               "frames_world_z": bb.DeviceBatch(b, num_iters=iters, mu=mu, cone=dict(projection="euclidean", normals=world_z)),
               "frames_slope": bb.DeviceBatch(b, num_iters=iters, mu=mu, cone=dict(projection="euclidean", normals=slope))}


def measure(args):
    from bunmpc_amd import _lib
    lib = _lib.lib()
    out = {config: measure_config(args, config) for config in CONFIGS}
    out["scratch_bytes_per_lane"] = {"frames_n_eff_4": lib.bmpc_biconvex_cone_frame_kernel_scratch_bytes(4), "frames_n_eff_2": lib.bmpc_biconvex_cone_frame_kernel_scratch_bytes(2),
                                     "cone_n_eff_4": lib.bmpc_biconvex_cone_kernel_scratch_bytes(4), "cone_n_eff_2": lib.bmpc_biconvex_cone_kernel_scratch_bytes(2)}
    return out


def measure_config(args, config):
    import torch
    from bunmpc_amd import _lib
    lib = _lib.lib()
    b, dev = legs(config, args.B, args.iters, args.mu, args.roll, args.pitch)
    out = {"config": config, "n_eff": b.E, "B": args.B, "H": b.H, "admm_iters": args.iters, "runs": args.runs, "mu": args.mu, "roll_deg": args.roll, "pitch_deg": args.pitch}
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
    for k in ("frames_world_z", "frames_slope"):
        out["ratio_%s_over_cone" % k] = out[k]["ms_median"] / out["cone"]["ms_median"]
        out["ratio_%s_per_fista_iteration" % k] = out[k]["ms_per_1000_fista_iters"] / out["cone"]["ms_per_1000_fista_iters"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--mu", type=float, default=0.3, help="the friction coefficient of every foot in every leg")
    ap.add_argument("--roll", type=float, default=10.0, help="roll of the slope leg's plane, degrees")
    ap.add_argument("--pitch", type=float, default=25.0, help="pitch of the slope leg's plane, degrees")
    ap.add_argument("--leg", choices=["measure"], help="(internal) run the measurement in this process and print its JSON")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.runs < 5:
        ap.error("--runs: at least five runs of each leg")
    if args.leg:
        print(json.dumps(measure(args)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--leg", "measure", "--runs", str(args.runs), "--warmup", str(args.warmup), "--B", str(args.B),
          "--iters", str(args.iters), "--mu", str(args.mu), "--roll", str(args.roll), "--pitch", str(args.pitch)]
    out = {"workload": "kernel about contact normals against the cone kernel (Euclidean friction-cone projection), harness form, one wave per SIMD", "date": time.strftime("%Y-%m-%d")}
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
