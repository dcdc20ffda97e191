"""Cost of keeping the trainers' data set on the device (bunmpc_amd/dataset_device.py) against the host hop it replaces.

Shape: the rows of one generator step, B = 4096 problems of R = 50 rows (43 + 12 + 5 + 12 doubles each), into a ring of --limit rows.
Legs, interleaved in one process (every sample of every leg follows a sample of the leg before it):

  append        DeviceDatabase.append of the four groups                                  events around --calls back-to-back calls
  append_scan   the same with drop_nonfinite (one more read of every kept row)            events around --calls back-to-back calls
  append_odd_slot  the same append into a ring that stands at an odd row (8-byte stores)  events around --calls back-to-back calls
  host          the parent path on the same tensors: .cpu().numpy() of the four groups
                plus dataset.Database.append into a host ring of the same size            host clock around one call, device idle before
  moments       calc_input_mean_std over the full ring                                    events around --moment-calls calls
  batch_4096    batch(index) at n = 4096, normalised cc rows, random indices              events around --calls calls
  batch_65536   ... at n = 65536
  step          one PlanLabelGenerator(goal_horizon=1).step at B = 4096                   events around one call
  step_append   the same step followed by append_step                                     events around one call

Per device leg the bytes the call must move, from the shapes (append: every kept element read once and written once, append_scan: read
twice; moments: two passes over states and cc_goals; batch: index, gathered row and written row), over its median time, and that rate
as a share of the machine's measured copy rate (--copy-rate, 6.29 TB/s on the MI355X).  One JSON line.

    python tools/dataset_bench.py [--runs 15] [--warmup 3] [--calls 200] [--moment-calls 20] [--limit 4000000] [--no-generator]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--moment-calls", type=int, default=20)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--R", type=int, default=50)
    ap.add_argument("--limit", type=int, default=4000000)
    ap.add_argument("--copy-rate", type=float, default=6.29e12, help="bytes per second read + written by a device copy")
    ap.add_argument("--no-generator", action="store_true")
    args = ap.parse_args()
    import torch
    from bunmpc_amd import dataset
    from bunmpc_amd.dataset_device import DeviceDatabase
    dev = "cuda:0"
    B, R, limit = args.B, args.R, args.limit
    widths = dict(states=43, actions=12, vc_goals=5, cc_goals=12)
    g = torch.Generator(device=dev).manual_seed(0)
    rows = {k: torch.randn((B, R, w), dtype=torch.float64, device=dev, generator=g) for k, w in widths.items()}
    db = DeviceDatabase(limit, goal_horizon=1, device=dev)
    host_db = dataset.Database(limit)
    for _ in range(-(-limit // (B * R))):          # fill the ring: the statistics and the batches run over all of it
        db.append(**rows)
    assert len(db) == limit
    db.calc_input_mean_std()
    index = {n: torch.randint(0, limit, (n,), device=dev, generator=g) for n in (4096, 65536)}
    row_bytes = 8 * sum(widths.values())
    moved = {"append": 2 * B * R * row_bytes, "append_scan": 3 * B * R * row_bytes, "moments": 2 * limit * 8 * (43 + 12),
             "batch_4096": 4096 * (8 + 2 * 8 * (43 + 12 + 12)), "batch_65536": 65536 * (8 + 2 * 8 * (43 + 12 + 12))}

    def host_append():
        h = {k: v.reshape(B * R, -1).cpu().numpy() for k, v in rows.items()}
        host_db.append(h["states"], h["actions"], vc_goals=h["vc_goals"], cc_goals=h["cc_goals"])

    # the same append into a ring that stands at an odd row: a 43-wide or 5-wide row then starts 8 bytes off a 16-byte boundary where
    # its source starts on one, so those groups are stored with 8-byte accesses
    odd = DeviceDatabase(limit, goal_horizon=1, device=dev)
    odd.append(**{k: v[0, :1] for k, v in rows.items()})
    moved["append_odd_slot"] = moved["append"]
    device_legs = {"append": (lambda: db.append(**rows), args.calls), "append_scan": (lambda: db.append(drop_nonfinite=True, **rows), args.calls),
                   "append_odd_slot": (lambda: odd.append(**rows), args.calls),
                   "moments": (db.calc_input_mean_std, args.moment_calls),
                   "batch_4096": (lambda: db.batch(index[4096]), args.calls), "batch_65536": (lambda: db.batch(index[65536]), args.calls)}
    if not args.no_generator:
        from bunmpc_amd import problems, urdf_model
        from bunmpc_amd.datagen import PlanLabelGenerator
        model = urdf_model.RobotModel.from_json(open(os.path.join(ROOT, "bunmpc_amd", "robots", "solo12.json")).read())
        gen = PlanLabelGenerator(model, goal_horizon=1, device=dev)
        q = torch.as_tensor(np.tile(problems.SOLO12_Q0, (B, 1)), device=dev)
        v = torch.zeros((B, 18), dtype=torch.float64, device=dev)
        t0 = torch.as_tensor(0.05 * (np.arange(B) % 3), device=dev)
        vd = torch.zeros((B, 3), dtype=torch.float64, device=dev)
        vd[:, 0] = 0.2
        step_db = DeviceDatabase(limit // 4, goal_horizon=1, device=dev)

        def step():
            return gen.step(q, v, t0, vd, generator=g, episode_length=200)
        device_legs["step"] = (step, 1)
        device_legs["step_append"] = (lambda: step_db.append_step(step()), 1)
    samples = {k: [] for k in list(device_legs) + ["host"]}
    for r in range(args.warmup + args.runs):
        for k, (call, calls) in device_legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                call()
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                samples[k].append(1e3 * e0.elapsed_time(e1) / calls)
        torch.cuda.synchronize()
        t = time.perf_counter()
        host_append()
        if r >= args.warmup:
            samples["host"].append(1e6 * (time.perf_counter() - t))
    out = {}
    for k, v in samples.items():
        out[k] = dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)))
        if k in moved:
            rate = moved[k] / (1e-6 * out[k]["median_us"])
            out[k].update(bytes=moved[k], TB_per_s=rate / 1e12, share_of_copy_rate=rate / args.copy_rate)
    ratios = {"host_over_append": out["host"]["median_us"] / out["append"]["median_us"],
              "host_over_append_scan": out["host"]["median_us"] / out["append_scan"]["median_us"]}
    if "step" in out:
        ratios["step_append_over_step"] = out["step_append"]["median_us"] / out["step"]["median_us"]
    print(json.dumps(dict(B=B, R=R, limit=limit, runs=args.runs, calls=args.calls, moment_calls=args.moment_calls, us_per_call=out, ratios=ratios)))


if __name__ == "__main__":
    main()
