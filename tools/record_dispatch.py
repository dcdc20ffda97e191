"""Record tests/golden/dispatch_table.json: which centroidal kernel every batch shape of tests/dispatch_rows.cases() gets.

Uses only the solve entry points and the "last launch" record (bmpc_biconvex_last_kernel_name, _last_lanes_per_problem,
_last_waves_per_simd), so it runs on any commit that has them -- the table is recorded on the commit BEFORE a change to the dispatch and
checked after it (tests/test_dispatch_plan_cpu.py, tests/test_dispatch_plan_gpu.py).  Needs the GPU; every row is one small solve.

    python tools/record_dispatch.py [--out tests/golden/dispatch_table.json] [--limit N]

--limit N records the first N rows only (a dry run to size a time limit from)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from tests import dispatch_rows as dr
    if not torch.cuda.is_available():
        sys.exit("record_dispatch needs a GPU")
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    cases = dr.cases()[:args.limit or None]
    rows, t0 = [], time.time()
    for i, c in enumerate(cases):
        row = dict(zip(dr.COLUMNS, c))
        rows.append(list(c) + list(dr.solve(row)))
        if i % 50 == 0:
            print("row %d / %d, %.0f s" % (i, len(cases), time.time() - t0), flush=True)
    out = args.out or dr.TABLE
    with open(out, "w") as f:
        f.write('{"simds": %d,\n "columns": %s,\n "rows": [\n' % (simds, json.dumps(list(dr.COLUMNS))))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print("%d rows in %.0f s -> %s" % (len(rows), time.time() - t0, out))


if __name__ == "__main__":
    main()
