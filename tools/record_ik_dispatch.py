"""Record tests/golden/ik_dispatch_table.json: which kernels, grids and workgroup sizes every host look of an IK-DDP batch solve launched.

    python tools/record_ik_dispatch.py [--out tests/golden/ik_dispatch_table.json] [--only NAME ...] [--keep DIR]

Every solve of tests/ik_dispatch_rows.solves() runs in a fresh child process (this file with --child NAME) under
`rocprofv3 --kernel-trace` with a time limit of its own; a child that fails ends the recording.  Only the solve entry point, the
bmpc_ik_set_* calls and the per-batch bmpc_ik_sched_t are used, so the tool runs on any commit that has them -- the table is recorded
on the commit BEFORE a change to the launch layer and must come out byte for byte the same after it (tests/test_ik_plan_cpu.py holds
bmpc_ik_plan_iteration to it).  Needs the GPU; each solve is a few milliseconds (the process around it a few seconds)."""
import argparse
import concurrent.futures
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOOP = ("ik_state_kernel", ("ik_calcdiff_kernel", "ik_calcdiff1_kernel"), ("ik_backward_kernel<1>", "ik_backward_kernel<2>"),
        ("ik_forward_kernel<1>", "ik_forward_kernel<2>", "ik_forward_kernel<3>"))


def child(name):
    from tests import ik_dispatch_rows as rows
    iters, last, digest = rows.run(rows.by_name(name))
    print("RESULT " + json.dumps({"iters_run": iters, "last_calcdiff": last, "digest": digest}), flush=True)


def launches(path):
    """[(short kernel name, workgroups, workgroup size)] of the trace's IK kernels, in dispatch order"""
    with open(path) as f:
        recs = list(csv.DictReader(f))
    recs.sort(key=lambda r: int(r["Dispatch_Id"]) if r.get("Dispatch_Id") else int(r["Start_Timestamp"]))
    out = []
    for r in recs:
        m = re.search(r"\b(ik_[a-z0-9_]+_kernel(?:<\d+>)?)", r["Kernel_Name"])
        if m:
            wg = int(r["Workgroup_Size_X"])
            assert int(r["Grid_Size_X"]) % wg == 0
            out.append((m.group(1), int(r["Grid_Size_X"]) // wg, wg))
    return out


def looks_of(seq, B, has_list):
    """the record of one solve from its launches (see tests/ik_dispatch_rows.py)"""
    assert [k[0] for k in seq].count("ik_init_kernel") == 1 and seq[0][0] == "ik_init_kernel", "one solve per trace"
    rec = dict(fused_direct=0, fused_grid=None, select_launches=0, express_launches=0, express_grid=None, looks=[])
    iters, it = [], 0           # iterations of the chunk being read: [state, derivative, Riccati, line search]
    for k in seq[1:]:
        name = k[0]
        if name == "ik_select_kernel":
            assert k[1:] == (1, 1024)
            rec["select_launches"] += 1
        elif name == "ik_fused_kernel":
            assert k[2] == 256
            if rec["select_launches"] == 0:
                assert not rec["looks"] and not iters and not rec["fused_direct"]
                rec["fused_direct"], rec["fused_grid"] = 1, k[1]
            else:
                assert rec["express_grid"] in (None, k[1])
                rec["express_launches"], rec["express_grid"] = rec["express_launches"] + 1, k[1]
        elif name == "ik_publish_active_kernel":
            if iters:
                assert all(i == iters[0] for i in iters), "one mapping per chunk"
                active = iters[0][2][1] if has_list else (B if len(rec["looks"]) < 2 else None)
                rec["looks"].append([it, active, len(iters)] + [list(x) for x in iters[0]])
                it += len(iters)
                iters = []
        elif name in LOOP[0] or any(name in group for group in LOOP[1:]):
            if not iters or len(iters[-1]) == 4:
                iters.append([])
            assert name == LOOP[0] if not iters[-1] else name in LOOP[len(iters[-1])], "state, derivative, Riccati, line search in turn"
            iters[-1].append(k)
    assert not iters and (rec["fused_direct"] == 0 or not rec["looks"])
    assert rec["select_launches"] == rec["express_launches"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", nargs="+")
    ap.add_argument("--keep", metavar="DIR", help="leave the traces under DIR (default: a temporary directory)")
    ap.add_argument("--jobs", type=int, default=4, help="child processes at a time")
    ap.add_argument("--time-limit", type=int, default=150, help="seconds per solve (process start, trace and all)")
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    from tests import ik_dispatch_rows as rows
    work = os.path.abspath(args.keep) if args.keep else tempfile.mkdtemp(prefix="ik_dispatch_")
    todo = [s for s in rows.solves() if not args.only or s[0] in args.only]

    def record(s):
        name, B, n_col, has_list, knob_values, sched = s
        d = os.path.join(work, name)
        cmd = ["timeout", "-k", "10", str(args.time_limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--child", name]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        result = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or len(result) != 1:
            return "%s: exit status %d\n%s" % (name, p.returncode, p.stdout[-4000:])
        traces = glob.glob(os.path.join(d, "**", "run_kernel_trace.csv"), recursive=True)
        assert len(traces) == 1, traces
        told = json.loads(result[0][len("RESULT "):])
        rec = dict(name=name, B=B, n_col=n_col, maxiter=rows.MAXITER, has_list=has_list, knobs=dict(rows.DEFAULTS, **knob_values),
                   sched={k: sched.get(k, 0) for k in rows.SCHED_FIELDS})
        rec.update(looks_of(launches(traces[0]), B, has_list))
        rec.update(iters_run=told["iters_run"], last_calcdiff=told["last_calcdiff"])
        print("%-30s %2d looks, %3d iterations run, fused-direct %d, express launches %d" %
              (name, len(rec["looks"]), rec["iters_run"], rec["fused_direct"], rec["express_launches"]), flush=True)
        return rec

    out = []
    for i in range(0, len(todo), args.jobs):         # a few children at a time; after a failure no further one is started
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            got = list(pool.map(record, todo[i:i + args.jobs]))
        failed = [g for g in got if isinstance(g, str)]
        if failed:
            sys.exit("\n".join(failed))
        out += got
    path = args.out or rows.TABLE
    with open(path, "w") as f:
        f.write('{"solves": [\n')
        for i, rec in enumerate(out):
            looks = rec.pop("looks")
            f.write(" " + json.dumps(rec)[:-1] + ', "looks": [\n')
            f.write(",\n".join("   " + json.dumps(lk) for lk in looks))
            f.write("\n  ]}" + (",\n" if i + 1 < len(out) else "\n"))
        f.write("]}\n")
    print("%d solves -> %s" % (len(out), path))


if __name__ == "__main__":
    main()
