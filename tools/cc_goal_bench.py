"""Cost of the contact-conditioned goals on the device (include/bunmpc_goals.h, csrc/cc_goals.hip).

Shape: Solo12 trot, B = 4096, episode_length = 3000 (a plan of 1200 knots, 480 switches per problem).  Two comparisons, one JSON line:

  arrays     bmpc_cc_goal_batch_device (the episode's plan walked, its schedule, the goal rows) against bmpc_plan_batch_device (the
             20-knot MPC plan of the same problems) on the same stream, interleaved, for max_rows = 50 (the rows a generator step
             labels) and max_rows = 3001 (the goals of the whole episode), with and without the plan written out;
  step       PlanLabelGenerator.step() with goal_horizon = 1 against the same step() with the option off (which launches what the
             generator launched before the option existed), interleaved, at --step-B problems.

Median, min and max of --runs launches each (torch events) after --warmup.  The GPU step runs in a child process under a time limit.

    python tools/cc_goal_bench.py [--runs 7] [--warmup 2] [--B 4096] [--episode-length 3000] [--step-B 4096]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 420


def timed(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    return dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)))


def interleaved(legs, args, torch):
    ms = {k: [] for k in legs}
    for r in range(args.warmup + args.runs):
        for k, fn in legs.items():
            t = timed(fn, torch)
            if r >= args.warmup:
                ms[k].append(t)
    return {k: stats(v) for k, v in ms.items()}


def measure(args):
    import torch
    from bunmpc_amd import problems, urdf_model
    from bunmpc_amd.cc_goal_batch import DeviceCcGoals, plan_knots
    from bunmpc_amd.plan_batch import DevicePlan
    gait, B, L = problems.TROT, args.B, args.episode_length
    b = problems.make_batch("solo12_trot", B)
    m = b.meta
    com = b.x_init[:, 0:3].copy()
    hip_off = np.broadcast_to(m["robot"].offsets_xy[None], (B, 4, 2)).copy()
    plan = DevicePlan(m["gait_objs"], m["robot"].offsets_xy, b.H, m["t0"], com, m["feet0_raw"], m["v_des"], m["w_des"], b.x_init)
    legs = {"plan_batch_h%d" % b.H: plan.build}
    goals = {}
    for rows, want_plan in ((50, False), (L + 1, False), (50, True)):
        name = "cc_goals_rows%d%s" % (rows, "_with_plan" if want_plan else "")
        goals[name] = DeviceCcGoals(gait, L, m["t0"], com, m["feet0_raw"], hip_off, m["v_des"], m["w_des"], goal_horizon=1, max_rows=rows,
                                    want_plan=want_plan)
        legs[name] = goals[name].build
    out = {"B": B, "episode_length": L, "plan_knots": plan_knots(L, gait), "arrays": interleaved(legs, args, torch)}
    g = goals["cc_goals_rows50"]
    out["arrays"]["switches_per_problem"] = float(g.counts.sum(dim=1).double().mean())
    out["arrays"]["status_nonzero"] = int((g.status != 0).sum())
    for k in goals:
        out["arrays"]["ratio_%s_over_plan_batch" % k] = out["arrays"][k]["ms_median"] / out["arrays"]["plan_batch_h%d" % b.H]["ms_median"]
    del goals, legs, plan, g
    torch.cuda.empty_cache()
    if args.step_B:
        from bunmpc_amd.datagen import PlanLabelGenerator
        model = urdf_model.RobotModel.from_json(open(os.path.join(ROOT, "bunmpc_amd", "robots", "solo12.json")).read())
        n = args.step_B
        wb = problems.make_wb_batch(model, n)
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")      # noqa: E731
        q, v = up(np.tile(problems.SOLO12_Q0, (n, 1))), torch.zeros((n, 18), dtype=torch.float64, device="cuda:0")
        t0, vd = up(wb.dyn.meta["t0"]), up(wb.dyn.meta["v_des_body"])
        gens = {"step_option_off": PlanLabelGenerator(model), "step_cc_goals": PlanLabelGenerator(model, goal_horizon=1, episode_length=L)}
        seeds = {k: torch.Generator(device="cuda:0").manual_seed(7) for k in gens}
        out["step"] = interleaved({k: (lambda k=k: gens[k].step(q, v, t0, vd, generator=seeds[k])) for k in gens}, args, torch)
        out["step"]["B"] = n
        out["step"]["ratio_cc_goals_over_option_off"] = out["step"]["step_cc_goals"]["ms_median"] / out["step"]["step_option_off"]["ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--episode-length", type=int, default=3000)
    ap.add_argument("--step-B", type=int, default=4096, help="batch of the PlanLabelGenerator.step() comparison (0: skip it)")
    ap.add_argument("--leg", choices=["measure"], help="(internal) run the measurement in this process and print its JSON")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.runs < 5:
        ap.error("--runs: at least five runs of each leg")
    if args.leg:
        print(json.dumps(measure(args)))
        return
    me = [sys.executable, os.path.abspath(__file__), "--leg", "measure", "--runs", str(args.runs), "--warmup", str(args.warmup), "--B", str(args.B),
          "--episode-length", str(args.episode_length), "--step-B", str(args.step_B)]
    out = {"workload": "contact-conditioned goals on the device against the MPC plan kernels and inside PlanLabelGenerator.step()",
           "date": time.strftime("%Y-%m-%d")}
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
