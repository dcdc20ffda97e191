"""Cost of turning logged contacts into cc_goals rows on the device (bunmpc_amd/contact_log.py::DeviceContactLog) against the bytes the
call must move.

Shape: B = 4096 logged episodes of T = 3000 steps with a trot-shaped contact pattern (period 500 steps, 60 % stance, the diagonal pairs
half a period apart), generated on the device.  Legs, interleaved in one process:

  copy                      a device-to-device copy of the log (ee_pos.clone(): read once, written once): the rate the others are shares of
  build_h<gh>               DeviceContactLog.build at goal horizon gh (1 and 3), failed-state test off
  build_h<gh>_failed        the same with q given as rows [q, v] of stride 37
  append                    DeviceDatabase.append of states, actions, vc_goals and given cc_goals, rows, keep         (goal horizon 1)
  build_append              build and append_episodes on the same stream
  host_twin                 contact_log.host_batch on --host-episodes of the same episodes: for scale, on whatever CPU runs it

Device legs: events around --calls back-to-back calls after --warmup calls, --runs samples, median and range.  Bytes a build must move,
from the shapes: the log read once (96 B T), com read once per goal row (16 rows: its x and y), the goals written once (96 gh max_rows:
the rows behind rows[b] are zeros that are written too), the schedule written once, q read once with the failed-state test (40 B T: five
doubles of a row).  One JSON line.

    python tools/contact_log_bench.py [--B 4096] [--T 3000] [--runs 15] [--warmup 3] [--calls 100] [--host-episodes 8]
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


def trot_log(torch, B, T, start, dev, period=500, stance=0.6):
    """ee_pos (B, T, 4, 3), com (B, T, 3) on the device"""
    f64 = dict(dtype=torch.float64, device=dev)
    o = (start[:, None] + torch.arange(T, device=dev)[None, :]).to(torch.float64)                      # (B, T)
    off = torch.tensor([0.0, 0.5, 0.5, 0.0], **f64)
    hips = torch.tensor([[0.195, 0.147], [0.195, -0.147], [-0.195, 0.147], [-0.195, -0.147]], **f64)
    u = o[:, :, None] / period + off[None, None, :]                                                    # (B, T, 4)
    cycle = torch.floor(u)
    standing = (u - cycle) < stance
    ee = torch.zeros((B, T, 4, 3), **f64)
    ee[..., 0] = hips[None, None, :, 0] + 0.15 * cycle + 0.01 * torch.sin(12.9898 * torch.arange(4, **f64)[None, None, :] + 78.233 * cycle)
    ee[..., 1] = hips[None, None, :, 1] + 0.005 * torch.cos(3.0 * cycle)
    ee[..., 2] = 1e-3
    ee *= standing[..., None]
    com = torch.stack([3e-4 * o + 2e-3 * torch.sin(0.013 * o), 1e-3 * torch.cos(0.007 * o), 0.23 + 1e-3 * torch.sin(0.005 * o)], dim=2)
    return ee.contiguous(), com.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--T", type=int, default=3000)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--host-episodes", type=int, default=8)
    ap.add_argument("--legs", default="", help="comma-separated leg names: only those (and the copy)")
    args = ap.parse_args()
    import torch
    from bunmpc_amd import contact_log
    from bunmpc_amd.dataset_device import DeviceDatabase
    dev = "cuda:0"
    B, T = args.B, args.T
    g = torch.Generator(device=dev).manual_seed(0)
    start = (torch.arange(B, device=dev) % 3 * 130).to(torch.int32)                                    # 0, 130, 260
    ee_pos, com = trot_log(torch, B, T, start, dev)
    x = torch.zeros((B, T, 37), dtype=torch.float64, device=dev)
    x[:, :, 2], x[:, :, 6] = 0.23, 1.0
    x[:, :, 3:5] = 0.02 * torch.randn((B, T, 2), dtype=torch.float64, device=dev, generator=g)
    episode_length = T
    logs = {gh: contact_log.DeviceContactLog(B, T, goal_horizon=gh, device=dev) for gh in (1, 3)}
    max_events = logs[1].max_events
    moved, legs = {"copy": 2 * ee_pos.numel() * 8}, {"copy": ee_pos.clone}
    for gh, log in logs.items():
        base = B * (T * 96 + T * 16 + 96 * gh * T + 16 * max_events * 8)
        moved["build_h%d" % gh], moved["build_h%d_failed" % gh] = base, base + B * T * 40
        legs["build_h%d" % gh] = (lambda log=log: log.build(ee_pos, com, start, episode_length))
        legs["build_h%d_failed" % gh] = (lambda log=log: log.build(ee_pos, com, start, episode_length, q=x[:, :, :19], gait_period=0.5))
    groups = dict(states=torch.randn((B, T, 43), dtype=torch.float64, device=dev, generator=g),
                  actions=torch.randn((B, T, 12), dtype=torch.float64, device=dev, generator=g),
                  vc_goals=torch.randn((B, T, 5), dtype=torch.float64, device=dev, generator=g))
    db = DeviceDatabase(B * T, goal_horizon=1, device=dev)
    logs[1].build(ee_pos, com, start, episode_length)
    torch.cuda.synchronize()
    rows, status = logs[1].rows.cpu().numpy(), logs[1].status.cpu().numpy()
    kept = int(rows[status == 0].sum())
    keep = (logs[1].status == 0).to(torch.int32)
    moved["append"] = 2 * kept * 8 * (43 + 12 + 5 + 12)
    moved["build_append"] = moved["build_h1"] + moved["append"]
    legs["append"] = lambda: db.append(cc_goals=logs[1].goals, rows=logs[1].rows, keep=keep, **groups)
    legs["build_append"] = lambda: db.append_episodes(groups["states"], groups["actions"], groups["vc_goals"], logs[1].build(ee_pos, com, start, episode_length))
    if args.legs:
        legs = {k: v for k, v in legs.items() if k == "copy" or k in args.legs.split(",")}
    samples = {k: [] for k in legs}
    for r in range(args.runs):
        for k, call in legs.items():
            for _ in range(args.warmup):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                call()
            e1.record()
            e1.synchronize()
            samples[k].append(1e3 * e0.elapsed_time(e1) / args.calls)
    out = {}
    for k, v in samples.items():
        out[k] = dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)), bytes=moved[k],
                      TB_per_s=moved[k] / (1e-6 * float(np.median(v))) / 1e12)
    for k in out:
        out[k]["share_of_copy_rate"] = out[k]["TB_per_s"] / out["copy"]["TB_per_s"]
    host = None
    if args.host_episodes:
        n = min(args.host_episodes, B)
        h = [t[:n].cpu().numpy() for t in (ee_pos, com, start)]
        t0 = time.perf_counter()
        tw = contact_log.host_batch(h[0], h[1], h[2], episode_length, goal_horizon=1, max_events=max_events)
        host = dict(episodes=n, seconds=time.perf_counter() - t0, seconds_per_episode=(time.perf_counter() - t0) / n,
                    equal_to_device=bool(np.array_equal(tw["goals"], logs[1].goals[:n].cpu().numpy()) and np.array_equal(tw["rows"], rows[:n])))
    print(json.dumps(dict(B=B, T=T, runs=args.runs, calls=args.calls, warmup=args.warmup, max_events=max_events, kept_rows=kept,
                          episodes_with_status=int((status != 0).sum()), rows_median=float(np.median(rows)), us_per_call=out, host_twin=host)))


if __name__ == "__main__":
    main()
