"""Cost of building the contact plan on a terrain height map: bmpc_plan_batch_terrain_device against bmpc_plan_batch_device.

Shape: solo12_trot, B = 4096, H = 20.  Legs, interleaved in one process, each a call of the entry point (its two kernels):

  flat          bmpc_plan_batch_device
  baseline      the same call of another build of the library (--baseline-lib, e.g. the parent commit's), loaded beside this one
  shared_map    the terrain call on one 256 x 256 map for the batch (512 KB: stays in L2)
  per_problem   the terrain call on one 64 x 64 map per problem (sheights = 4096; 128 MB in all)

The plan kernels are microseconds long, so a timed sample is --calls back-to-back calls between two events; one JSON line with the
median, min and max over --runs samples per leg, in microseconds per call, and the ratios of the medians to `flat`.

    python tools/terrain_plan_bench.py [--runs 15] [--warmup 3] [--calls 2000] [--B 4096] [--baseline-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--baseline-lib")
    args = ap.parse_args()
    import torch
    from bunmpc_amd import _lib, problems
    from bunmpc_amd.plan_batch import DevicePlan
    from bunmpc_amd.terrain import HeightMap
    lib = _lib.lib()
    b = problems.make_batch("solo12_trot", args.B)
    m = b.meta
    rng = np.random.default_rng(1)
    maps = {"flat": None,
            "shared_map": HeightMap(-1.0, -1.0, 0.01, 0.03 * rng.standard_normal((256, 256))),
            "per_problem": HeightMap(-1.0, -1.0, 0.04, 0.03 * rng.standard_normal((args.B, 64, 64)))}
    plans = {k: DevicePlan(m["gait_objs"], m["robot"].offsets_xy, b.H, m["t0"], b.x_init[:, 0:3].copy(), m["feet0_raw"], m["v_des"], m["w_des"],
                           b.x_init, terrain=hm) for k, hm in maps.items()}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    legs = {k: p.build for k, p in plans.items()}
    if args.baseline_lib:
        base = C.CDLL(args.baseline_lib)
        base.bmpc_plan_batch_device.restype, base.bmpc_plan_batch_device.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        flat = plans["flat"]

        def baseline():
            if base.bmpc_plan_batch_device(C.byref(flat.desc), stream) != _lib.OK:
                raise RuntimeError("baseline library refused the plan")
        legs["baseline"] = baseline
        want = flat.build().cnt_plan.clone()
        flat.cnt_plan.zero_()
        baseline()
        assert torch.equal(flat.cnt_plan, want), "the baseline library builds another plan"
    samples = {k: [] for k in legs}
    for r in range(args.warmup + args.runs):
        for k, call in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                call()
            t1.record()
            t1.synchronize()
            if r >= args.warmup:
                samples[k].append(1e3 * t0.elapsed_time(t1) / args.calls)
    out = {k: dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v))) for k, v in samples.items()}
    for k in out:
        out[k]["ratio_to_flat"] = out[k]["median_us"] / out["flat"]["median_us"]
    print(json.dumps(dict(B=args.B, H=b.H, runs=args.runs, calls=args.calls, us_per_call=out)))


if __name__ == "__main__":
    main()
