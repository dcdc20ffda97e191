"""Is the device code of the library the same in two source trees?  Kernel by kernel, wherever the kernel lives.

    python tools/device_asm_diff.py PARENT_TREE THIS_TREE [--keep DIR] [--units admm_band_f64_e4 ik_ddp ...]

Every job of each tree's own bunmpc_amd/build.py (compile_jobs(); a tree from before that function: its SOURCES with FILE_FLAGS) is
compiled to gfx950 assembly with the job's flags plus --cuda-device-only -S; --units keeps the jobs of these names, in either tree.
The listings are not compared file against file: kernels move between units, host templates that move reorder the kernels within a
unit, which renumbers the function index of local labels (.LBB<n>_<m>), and the __hip_cuid_* symbol differs on every compilation.
Instead every kernel's text -- from its symbol label to its .end_amdhsa_kernel -- and its entry in the metadata note are cut out by
name, comments are dropped, the function index in local labels is replaced by a placeholder, and the two trees are compared symbol by
symbol.  One line per kernel with its unit on each side, `same` or `DIFFERS`; a kernel that exists on one side only is a difference.
Exit status 0 only if every kernel is the same."""
import argparse
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys
import tempfile


def jobs_of(tree):
    """[(job name, hipcc command without output options)] of a tree, by its own build.py"""
    spec = importlib.util.spec_from_file_location("_build_of_tree", os.path.join(tree, "bunmpc_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    if hasattr(b, "compile_jobs"):
        return [(j[0], b.compile_cmd(j)) for j in b.compile_jobs()]
    return [(s, [b.HIPCC] + b.FLAGS + b.FILE_FLAGS.get(s, []) + [os.path.join(b.CSRC, s)]) for s in b.SOURCES]


def kernels_of(path):
    """{kernel symbol: normalised text + metadata entry} of one listing"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n", text, re.M):
        name = m.group(1)
        start = text.index("\n%s:" % name) + 1
        end = text.index("\t.end_amdhsa_kernel\n", m.end()) + len("\t.end_amdhsa_kernel\n")
        out[name] = text[start:end]
    if not out:      # (a unit of host code)
        return {}
    meta = text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")]
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)$", entry, re.M).group(1)
        out[name] += "---- metadata\n" + entry
    # comments go (they repeat the function index: "in Loop: Header=BB8_25", padded to a column), local labels lose that index
    return {k: re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1N", re.sub(r"[ \t]*;.*$", "", v, flags=re.M)) for k, v in out.items()}


def kernels_of_tree(listings):
    """{kernel symbol: (unit, text)} over [(unit, path of its listing)]; a symbol that two units of one tree define is an error"""
    out = {}
    for unit, path in listings:
        for name, text in kernels_of(path).items():
            if name in out:
                raise ValueError("%s is in %s and in %s" % (name, out[name][0], unit))
            out[name] = (unit, text)
    return out


def compare(parent, this):
    """[(kernel symbol, its unit in the parent tree or None, in this tree or None, verdict)] of two kernels_of_tree()"""
    rows = []
    for name in sorted(set(parent) | set(this)):
        a, b = parent.get(name), this.get(name)
        verdict = "DIFFERS (only in the %s tree)" % ("parent" if a else "this") if not (a and b) else ("same" if a[1] == b[1] else "DIFFERS")
        rows.append((name, a and a[0], b and b[0], verdict))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_tree")
    ap.add_argument("this_tree")
    ap.add_argument("--keep", metavar="DIR", help="leave the .s files under DIR/parent and DIR/this (default: a temporary directory)")
    ap.add_argument("--units", nargs="+", help="job names (default: every job of each tree)")
    args = ap.parse_args()
    work = args.keep or tempfile.mkdtemp(prefix="device_asm_")
    listings, cmds = {}, []
    for side, tree in (("parent", args.parent_tree), ("this", args.this_tree)):
        os.makedirs(os.path.join(work, side), exist_ok=True)
        listings[side] = []
        for name, cmd in jobs_of(os.path.abspath(tree)):
            if args.units is None or name in args.units:
                listings[side].append((name, os.path.join(work, side, name + ".s")))
                cmds.append(cmd + ["--cuda-device-only", "-S", "-o", listings[side][-1][1]])
    with concurrent.futures.ThreadPoolExecutor(max_workers=16) as pool:
        for cmd, status in zip(cmds, pool.map(subprocess.call, cmds)):
            if status != 0:
                sys.exit("hipcc failed: " + " ".join(cmd))
    parent, this = kernels_of_tree(listings["parent"]), kernels_of_tree(listings["this"])
    rows = compare(parent, this)
    if not rows:
        sys.exit("no kernel in either tree: do the --units name jobs?")
    for name, ua, ub, verdict in rows:
        print("%-24s %-24s %-8s %s" % (ua or "-", ub or "-", verdict, name))
    differing = sum(verdict != "same" for _, _, _, verdict in rows)
    print("%d kernels in the parent tree, %d in this tree, %d differ" % (len(parent), len(this), differing))
    print("all same" if differing == 0 else "%d kernels DIFFER" % differing)
    sys.exit(1 if differing else 0)


if __name__ == "__main__":
    main()
