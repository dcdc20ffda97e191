#!/usr/bin/env python3
"""VALU instructions of one loop-nest level of a kernel, by the SOURCE LINE they were compiled from: what the ADMM-loop body of the
headline kernel (level 1: everything of an ADMM iteration outside the FISTA loops) spends its instructions on.

    python tools/phase_lines.py --compile admm_diag_f64_e4 KERNEL_SUBSTRING [--level N] [--file biconvex_admm_body.h] [--ranges name:lo-hi,...]

The unit is compiled with its own flags (bunmpc_amd/build.py) and -gline-tables-only, which adds `.loc file line col` markers to the
listing and leaves the instructions what they are (the totals are those of tools/phase_waits.py).  An instruction belongs to the line
of the last marker in front of it; an inlined helper's instructions carry the helper's line, so lines of other files are summed per
file.  Without --ranges: one row per source line of --file with at least one instruction; with it: one row per named range of lines,
and `other` for the rest."""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phase_waits as pw  # noqa: E402


def compile_listing(job):
    sys.path.insert(0, pw.ROOT)
    from bunmpc_amd import build
    out = os.path.join(tempfile.mkdtemp(), job + ".s")
    cmd = build.compile_cmd(build.job(job)) + ["--cuda-device-only", "-S", "-gline-tables-only", "-I", os.path.join(pw.ROOT, "include"), "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out


def main():
    argv = sys.argv[1:]

    def opt(name, default):
        if name in argv:
            v = argv[argv.index(name) + 1]
            del argv[argv.index(name):argv.index(name) + 2]
            return v
        return default
    level, want, ranges = int(opt("--level", "1")), opt("--file", "biconvex_admm_body.h"), opt("--ranges", "")
    args = [a for a in argv if not a.startswith("--")]
    listing = compile_listing(args[0]) if "--compile" in argv else args[0]
    lines = open(listing).read().split("\n")
    files = {}
    for l in lines:
        m = re.match(r'^\s+\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', l)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(2))
    body = pw.kernel_body(lines, args[1])
    depth, where = 0, ("?", 0)
    valu, instr = collections.Counter(), collections.Counter()
    k = 0
    while k < len(body):
        l = body[k]
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", l) or re.match(r"^; (%bb\.\d+):(.*)$", l)
        if m:
            depth = 0
            notes = [m.group(2)]
            while k + 1 < len(body) and re.match(r"^\s+;", body[k + 1]):
                k += 1
                notes.append(body[k])
            for n in notes:
                h = re.search(r"in Loop: Header=BB\d+_\d+ Depth=(\d+)", n) or re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", n)
                if h:
                    depth = int(h.group(1))
            k += 1
            continue
        m = re.match(r"^\s+\.loc\s+(\d+)\s+(\d+)", l)
        if m:
            where = (files.get(int(m.group(1)), m.group(1)), int(m.group(2)))
        t = l.split(";")[0].strip()
        if depth == level and t and not t.startswith(".") and not t.endswith(":"):
            instr[where] += 1
            valu[where] += pw.is_valu(t.split()[0])
        k += 1
    print("level %d: %d instructions, %d VALU" % (level, sum(instr.values()), sum(valu.values())))
    if ranges:
        named = [(n, int(a), int(b)) for n, a, b in (re.match(r"(.+):(\d+)-(\d+)$", r).groups() for r in ranges.split(","))]
        acc = collections.OrderedDict((n, [0, 0]) for n, _, _ in named)
        acc["other"] = [0, 0]
        for (f, ln), c in instr.items():
            key = next((n for n, a, b in named if f == want and a <= ln <= b), "other")
            acc[key][0] += c
            acc[key][1] += valu[(f, ln)]
        for n, (i, v) in acc.items():
            print("%-40s instr %5d  VALU %5d" % (n, i, v))
        return
    other = collections.Counter()
    for (f, ln), c in sorted(instr.items()):
        if f == want:
            print("%s:%-5d instr %4d  VALU %4d" % (f, ln, c, valu[(f, ln)]))
        else:
            other[f] += valu[(f, ln)]
    for f, v in other.items():
        print("%-30s VALU %5d" % (f, v))


if __name__ == "__main__":
    main()
