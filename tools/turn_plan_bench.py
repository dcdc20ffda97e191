"""Cost of turning commands in the whole-body plan builder: bmpc_wb_plan_batch_turn_device against bmpc_wb_plan_batch_device, and
PlanLabelGenerator.step(w_des=...) against step().

Shape: Solo12 trot, B = 4096, H = 20, T = 10, the states of problems.make_wb_batch, every command != 0.  Legs, interleaved in one
process, each a call of the entry point (its four kernels):

  plain         bmpc_wb_plan_batch_device
  plain_again   the same call on a second set of tensors: the difference of the two medians, with the min / max of each, is the spread
                a difference between legs has to leave before it means anything
  baseline      the same call of another build of the library (--baseline-lib, e.g. the parent commit's), loaded beside this one, on
                the same states; its plan must equal `plain`'s, bit for bit
  turn          bmpc_wb_plan_batch_turn_device
  turn_zero     the same with every command 0 (the branch not taken)

The plan kernels are tens of microseconds long, so a timed sample is --calls back-to-back calls between two events; the median, min and
max over --runs samples per leg, in microseconds per call, and the ratios of the medians to `plain`.

--step: PlanLabelGenerator.step (perturb=False, goal_horizon=1) with and without w_des, --step-runs samples of one call each between
two events, in milliseconds (step_plain, step_plain_again, step_turn).  With a library that has no turn entry points (BUNMPC_LIB=<the
parent's build>) only the plain legs run: that is how the parent's step() is timed, in a process of its own.

One JSON line.

    python tools/turn_plan_bench.py [--runs 15] [--warmup 3] [--calls 500] [--B 4096] [--baseline-lib PATH] [--step] [--step-runs 15]
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

OUT = ("x_init", "cnt_plan", "swing_time", "dt", "X_nom", "X_ter", "ik_tasks")


def stats(samples, unit, ref):
    out = {k: {"median_" + unit: float(np.median(v)), "min_" + unit: float(np.min(v)), "max_" + unit: float(np.max(v))} for k, v in samples.items()}
    for k in out:
        out[k]["ratio_to_" + ref] = out[k]["median_" + unit] / out[ref]["median_" + unit]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--baseline-lib")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-runs", type=int, default=15)
    args = ap.parse_args()
    import torch
    from bunmpc_amd import _lib, fk_np, problems, urdf_model
    from bunmpc_amd.cyclic_gen import composite_inertia_base
    from bunmpc_amd.inverse_kinematics_cpp import DeviceModel
    from bunmpc_amd.plan_batch import DeviceWbPlan
    if not torch.cuda.is_available():
        raise SystemExit("tools/turn_plan_bench.py needs a GPU")
    lib = _lib.lib()
    has_turn = hasattr(lib, "bmpc_wb_plan_batch_turn_device")
    model = urdf_model.RobotModel.from_json(open(os.path.join(ROOT, "bunmpc_amd", "robots", "solo12.json")).read())
    B = args.B
    wb = problems.make_wb_batch(model, B)
    t0, vb = wb.dyn.meta["t0"], wb.dyn.meta["v_des_body"]
    rng = np.random.default_rng(2)
    w_des = rng.uniform(0.1, 0.5, B) * rng.choice([-1.0, 1.0], B)          # every problem turns
    Izz = float(composite_inertia_base(model, problems.SOLO12_Q0)[2, 2])
    k0 = fk_np.kinematics(model, problems.SOLO12_Q0[None])
    offs = np.round(fk_np.frame_positions(model, k0, problems.HIPS)[0] - k0["com"][0], 3)
    offs[:, 1] += np.array([0.04, -0.04, 0.04, -0.04])

    def plan(dm, **kw):
        return DeviceWbPlan(dm, problems.TROT, offs[:, :2], problems.FEET, problems.TROT_IK, wb.x, t0, vb, wb.dyn.H, wb.ik_T, **kw)

    dm = DeviceModel(model)
    plans = {"plain": plan(dm), "plain_again": plan(dm)}
    if has_turn:
        plans["turn"] = plan(dm, w_des=w_des, yaw_inertia=Izz)
        plans["turn_zero"] = plan(dm, w_des=np.zeros(B), yaw_inertia=Izz)
    legs = {k: p.build for k, p in plans.items()}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    want = {k: getattr(plans["plain"].build(), k).clone() for k in OUT}
    if args.baseline_lib:
        base = C.CDLL(args.baseline_lib)
        for name in ("bmpc_model_create", "bmpc_model_destroy", "bmpc_wb_plan_batch_device"):
            getattr(base, name).restype, getattr(base, name).argtypes = _lib._SIGS[name]
        base_plan = plan(DeviceModel(model, lib=base))      # the baseline's own model handle

        def baseline():
            if base.bmpc_wb_plan_batch_device(C.byref(base_plan.desc), stream) != _lib.OK:
                raise RuntimeError("baseline library refused the plan")
        legs["baseline"] = baseline
        baseline()
        for k in OUT:
            assert torch.equal(getattr(base_plan, k), want[k]), "the baseline library builds another %s" % k
    if has_turn:
        zero = plans["turn_zero"].build()
        for k in OUT:
            assert torch.equal(getattr(zero, k), want[k]), "commands that are all 0 change %s" % k
        turned = plans["turn"].build()
        assert not torch.equal(turned.X_nom, want["X_nom"]) and bool(torch.isfinite(turned.X_nom).all())
    samples = {k: [] for k in legs}
    for r in range(args.warmup + args.runs):
        for k, call in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                call()
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                samples[k].append(1e3 * e0.elapsed_time(e1) / args.calls)
    res = dict(B=B, H=wb.dyn.H, T=wb.ik_T, runs=args.runs, calls=args.calls, library=os.environ.get("BUNMPC_LIB", "this build"),
               us_per_call=stats(samples, "us", "plain"))
    if args.step:
        from bunmpc_amd.datagen import PlanLabelGenerator
        dev = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda:0")      # noqa: E731
        q, v, t, vd, w = dev(wb.x[:, :19]), dev(wb.x[:, 19:]), dev(t0), dev(vb), dev(w_des)
        gens = {"step_plain": (PlanLabelGenerator(model, goal_horizon=1), {}), "step_plain_again": (PlanLabelGenerator(model, goal_horizon=1), {})}
        if has_turn:
            gens["step_turn"] = (PlanLabelGenerator(model, goal_horizon=1), dict(w_des=w))
        ssamples = {k: [] for k in gens}
        for r in range(args.warmup + args.step_runs):
            for k, (gen, kw) in gens.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gen.step(q, v, t, vd, perturb=False, episode_length=600, **kw)
                e1.record()
                e1.synchronize()
                if r >= args.warmup:
                    ssamples[k].append(e0.elapsed_time(e1))
        res.update(step_runs=args.step_runs, ms_per_step=stats(ssamples, "ms", "step_plain"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
