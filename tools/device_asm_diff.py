"""Is the device code of the kernel units (the twelve centroidal ADMM units and ik_ddp.hip) the same in two source trees?  Kernel by kernel.

    python tools/device_asm_diff.py PARENT_TREE THIS_TREE [--keep DIR] [--units biconvex_admm_kq.hip ik_ddp.hip ...]

Each unit (any source of bunmpc_amd/csrc may be named) is compiled in both trees to gfx950 assembly with the tree's own flags (bunmpc_amd/build.py: FLAGS and
FILE_FLAGS, plus --cuda-device-only -S).  The files are not compared with diff: host templates that move reorder the kernels within a
file, which renumbers the function index of local labels (.LBB<n>_<m>), and the __hip_cuid_* symbol differs on every compilation.
Instead every kernel's text -- from its symbol label to its .end_amdhsa_kernel -- and its entry in the metadata note are cut out by
name, comments are dropped, the function index in local labels is replaced by a placeholder, and the two sides are compared.  One line per kernel, `same` or
`DIFFERS`; a kernel that exists on one side only is a difference (so is every kernel of a unit whose source one tree does not have).
Exit status 0 only if every kernel of every unit is the same."""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

UNITS = ["biconvex_admm.hip", "biconvex_admm_e2.hip", "biconvex_admm_bq.hip", "biconvex_admm_bq_e2.hip", "biconvex_admm_kq.hip", "biconvex_admm_kq_e2.hip",
         "biconvex_admm_cone.hip", "biconvex_admm_cone_e2.hip", "biconvex_admm_conef.hip", "biconvex_admm_conef_e2.hip", "biconvex_admm_f32.hip", "biconvex_admm_f32_e2.hip", "ik_ddp.hip"]


def build_settings(tree):
    spec = importlib.util.spec_from_file_location("_build_of_tree", os.path.join(tree, "bunmpc_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_units(tree, units, out_dir):
    """start hipcc -S for every unit of the tree; returns [(unit, path, process)], process None for a unit the tree does not have"""
    b = build_settings(tree)
    os.makedirs(out_dir, exist_ok=True)
    jobs = []
    for u in units:
        path = os.path.join(out_dir, u.replace(".hip", ".s"))
        src = os.path.join(tree, "bunmpc_amd", "csrc", u)
        cmd = [b.HIPCC] + b.FLAGS + b.FILE_FLAGS.get(u, []) + ["--cuda-device-only", "-S", src, "-o", path]
        jobs.append((u, path, subprocess.Popen(cmd) if os.path.exists(src) else None))
    return jobs


def kernels_of(path):
    """{kernel symbol: normalised text + metadata entry}"""
    if not os.path.exists(path):      # (the tree has no such unit)
        return {}
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n", text, re.M):
        name = m.group(1)
        start = text.index("\n%s:" % name) + 1
        end = text.index("\t.end_amdhsa_kernel\n", m.end()) + len("\t.end_amdhsa_kernel\n")
        out[name] = text[start:end]
    meta = text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")]
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)$", entry, re.M).group(1)
        out[name] += "---- metadata\n" + entry
    # comments go (they repeat the function index: "in Loop: Header=BB8_25", padded to a column), local labels lose that index
    return {k: re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1N", re.sub(r"[ \t]*;.*$", "", v, flags=re.M)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_tree")
    ap.add_argument("this_tree")
    ap.add_argument("--keep", metavar="DIR", help="leave the .s files under DIR/parent and DIR/this (default: a temporary directory)")
    ap.add_argument("--units", nargs="+", default=UNITS)
    args = ap.parse_args()
    work = args.keep or tempfile.mkdtemp(prefix="device_asm_")
    jobs = {side: compile_units(os.path.abspath(tree), args.units, os.path.join(work, side))
            for side, tree in (("parent", args.parent_tree), ("this", args.this_tree))}
    for side in jobs:
        for u, path, p in jobs[side]:
            if p is not None and p.wait() != 0:
                sys.exit("hipcc failed on %s of the %s tree" % (u, side))
    differing = 0
    for (u, pa, _), (_, th, _) in zip(jobs["parent"], jobs["this"]):
        a, b = kernels_of(pa), kernels_of(th)
        bad = 0
        for name in sorted(set(a) | set(b)):
            verdict = "same" if a.get(name) == b.get(name) else ("DIFFERS" if name in a and name in b else "DIFFERS (only in the %s tree)" % ("parent" if name in a else "this"))
            bad += verdict != "same"
            print("%-26s %-8s %s" % (u, verdict, name))
        print("%-26s %d kernels in the parent tree, %d in this tree, %d differ" % (u, len(a), len(b), bad))
        differing += bad
    print("all same" if differing == 0 else "%d kernels DIFFER" % differing)
    sys.exit(1 if differing else 0)


if __name__ == "__main__":
    main()
