"""Cost of a Q that couples neighbouring knots (force-rate, momentum-rate terms): the band-cost kernel against the diagonal raw-form
kernel on the same problems.

Shape: solo12_trot (four feet) and biped_walk (two feet), B = 4096, H = 20, raw form, 10 ADMM iterations, cold start, fp64, one wave
per SIMD forced for both (the band kernel has no two-waves build, so like is compared with like).  The diagonal leg solves the batch's
own raw arrays; the band leg the rate costs problems.rate_costs makes of them (lam_f = lam_x = 0.5) -- another problem, so the FISTA
iteration counts differ and the times are also given per 1000 FISTA iterations.  (The diagonal kernel is this tree's: the band
instantiations are translation units of their own and leave its instructions what they were.)  One JSON line:

  events     per foot count the two legs interleaved in one process, median, min and max of --runs launches each (torch events)
  profile    the kernels' own times from a rocprofv3 --kernel-trace --stats run of its own (median per kernel over its launches)

Every GPU step runs in a child process under a time limit; the first that fails ends the run.

    python tools/band_cost_bench.py [--runs 7] [--warmup 2] [--B 4096] [--iters 10] [--no-profile]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 300


CONFIGS = ("solo12_trot", "biped_walk")
LAM = 0.5


def legs(config, B, iters):
    from bunmpc_amd import batch as bb
    from bunmpc_amd import problems
    from oracle import oracle_c
    oracle_c.build()
    b = problems.make_batch(config, B)
    pre = oracle_c.solve_batch(b, num_iters=0)
    raw = {k: pre[k] for k in ("Qx", "qx", "lbx", "ubx", "Qf")}
    rc = problems.rate_costs(pre["Qx"], pre["Qf"], b.E, lam_x=LAM, lam_f=LAM)
    return b, {"diagonal": bb.DeviceBatch(b, num_iters=iters, raw=raw), "band": bb.DeviceBatch(b, num_iters=iters, raw=dict(raw, **rc))}


def measure(args):
    return {config: measure_config(args, config) for config in CONFIGS}


def measure_config(args, config):
    import torch
    from bunmpc_amd import _lib
    lib = _lib.lib()
    lib.bmpc_set_two_waves_per_simd(0)
    lib.bmpc_set_latency_mapping_max_batch(0)
    b, dev = legs(config, args.B, args.iters)
    out = {"config": config, "n_eff": b.E, "B": args.B, "H": b.H, "admm_iters": args.iters, "runs": args.runs, "lam_f": LAM, "lam_x": LAM}
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
    out["ratio_band_over_diagonal"] = out["band"]["ms_median"] / out["diagonal"]["ms_median"]
    out["ratio_per_fista_iteration"] = out["band"]["ms_per_1000_fista_iters"] / out["diagonal"]["ms_per_1000_fista_iters"]
    # the spread of the ratio over the repeated runs: the extremes of band / diagonal, per FISTA iteration
    f = out["diagonal"]["fista_iters_per_solve"] / out["band"]["fista_iters_per_solve"]
    out["ratio_per_fista_iteration_range"] = [f * out["band"]["ms_min"] / out["diagonal"]["ms_max"], f * out["band"]["ms_max"] / out["diagonal"]["ms_min"]]
    return out


def profile_summary(directory):
    """median duration per kernel and foot count of the ADMM launches in a rocprofv3 kernel trace"""
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    out = {}
    for feet, lanes in ((4, 32), (2, 32)):      # (H = 20 at B = 4096: 32 lanes per problem)
        o = {}
        for leg, word in (("diagonal", "biconvex_admm_kernel<double, %d, %d," % (lanes, feet)), ("band", "biconvex_admm_kq_kernel<%d, %d," % (lanes, feet))):
            d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if word in r["Kernel_Name"]]
            if d:
                o[leg] = {"launches": len(d), "kernel_ms_median": float(np.median(d)), "kernel_ms_min": float(np.min(d))}
        if len(o) == 2:
            o["ratio_band_over_diagonal"] = o["band"]["kernel_ms_median"] / o["diagonal"]["kernel_ms_median"]
        out["n_eff_%d" % feet] = o
    out["kernels_seen"] = sorted({r["Kernel_Name"][:60] for r in rows if "biconvex_admm" in r["Kernel_Name"]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--leg", choices=["measure"], help="(internal) run the measurement in this process and print its JSON")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.runs < 5:
        ap.error("--runs: at least five runs of each leg")
    if args.leg:
        print(json.dumps(measure(args)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--leg", "measure", "--runs", str(args.runs), "--warmup", str(args.warmup), "--B", str(args.B),
          "--iters", str(args.iters)]
    out = {"workload": "band-cost kernel (costs between neighbouring knots) against the diagonal raw-form kernel, one wave per SIMD", "date": time.strftime("%Y-%m-%d")}
    steps = [("events", me, None)]
    tmp = tempfile.mkdtemp(prefix="band_cost_prof_")
    if not args.no_profile:
        steps.append(("profile", ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--"] + me, tmp))
    for name, cmd, prof_dir in steps:
        try:
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=TIMEOUT_S)
        except subprocess.TimeoutExpired:
            out[name] = {"error": "timed out after %d s" % TIMEOUT_S}
            break
        if p.returncode != 0:
            out[name] = {"error": "exit status %d" % p.returncode, "stderr_tail": p.stderr[-800:]}
            break
        out[name] = profile_summary(prof_dir) if prof_dir else json.loads(p.stdout.strip().splitlines()[-1])
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))
    if any("error" in v for v in out.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
