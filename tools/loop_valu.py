#!/usr/bin/env python3
"""Vector instructions per loop of one kernel in a hipcc -S listing.  Every innermost loop (a block range closed by a backward branch:
the FISTA iteration bodies) with the vector (VALU) instructions it holds in all -- DPP moves, permlanes, readlanes and conversions included,
memory and scalar instructions not -- and the same on the cheapest path through the body (from its head to its back edge: an
iteration that takes none of the branches it can skip -- the cone step, the retry bookkeeping, the fp64 fall-back of the step
decisions), with that path's fp64 arithmetic (v_fma_f64, v_fmac_f64, v_mul_f64, v_add_f64), DPP moves, DPP-fused operations and
permlanes.  Also the kernel's registers, scratch and static LDS as the compiler reports them.

    python tools/loop_valu.py LISTING.s KERNEL_SUBSTRING [--through RE]... [--committing] [--momentum] [--scalar] [--blocks] [--mnemonics]
    python tools/loop_valu.py --compile admm_diag_f64_e4 KERNEL_SUBSTRING [--through RE]... [--committing] [--momentum] [--scalar] [--blocks] [--mnemonics]
        (--compile: device code of that job of bunmpc_amd/build.py, with its flags; --through RE: the cheapest path that runs an
        instruction matching RE, e.g. 'permlane' for an iteration that reduces its sums -- in fp32 where it can; given more than
        once: a path that runs an instruction of every RE, each in a block of its own; --committing: --through ds_write2, the
        iteration that writes x_{k+1} and its image back to LDS.  The plain cheapest path of a certified loop is NOT an iteration
        that commits: it leaves the loop before applyA(xn), the momentum step and the write-back.  The headline kernel's certified
        loops: --committing is the screened iteration, --committing --through permlane16 the one that takes the fp32 sum; in the
        force loop, whose two unrolled copies are one loop here, the path runs one copy and leaves by the other's exit test;
        --mnemonics: the path's vector instructions counted by mnemonic -- is a select or a mask operation on it?
        --momentum: --through the re-read of the loop constants' first pair (`ds_read2_b64 ... offset1:1`), which the loop-constants
        build issues at the head of its momentum step: the iteration that commits in `biconvex_admm_clds_kernel`, whose only
        ds_write2 is the rare latch; --momentum alone is the settled iteration, --momentum --through permlane16 the one that
        takes the fp32 sum; with it the path also runs every exec-masked region it meets (no s_cbranch_execz edge), as the hardware
        does while one lane is in it -- the rvalid half of the motion loop's momentum step is such a region;
        --scalar: the path's instructions that are NOT vector ALU, by class -- SALU (arithmetic, compares, selects, moves, mask
        operations), branches, s_waitcnt, s_nop, scalar memory, LDS, vector memory, other -- and the SALU ones by mnemonic.  In an
        issue-bound kernel with two waves per SIMD each of them is an issue turn that is not a VALU turn.)

The headline kernel: 'biconvex_admm_kernelIdLi32ELi4ELb0ELb0ELi2E' (biconvex_admm_kernel<double, 32, 4, false, false, 2>)."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = ("v_fma_f64", "v_fmac_f64", "v_mul_f64", "v_add_f64")
NOT_VALU = ("global_", "buffer_", "flat_", "scratch_", "ds_", "s_")


def compile_listing(job):
    sys.path.insert(0, ROOT)
    from bunmpc_amd import build
    out = os.path.join(tempfile.mkdtemp(), job + ".s")
    cmd = build.compile_cmd(build.job(job)) + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"), "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out


def is_valu(mn):
    return mn.startswith("v_") and not mn.startswith(NOT_VALU)


def scalar_class(mn):
    """the class of an instruction that is not VALU, as --scalar reports it"""
    if mn.startswith(("s_branch", "s_cbranch")):
        return "branch"
    if mn.startswith("s_waitcnt"):
        return "s_waitcnt"
    if mn.startswith("s_nop"):
        return "s_nop"
    if mn.startswith(("s_load", "s_buffer_load", "s_scratch_load")):
        return "scalar memory"
    if mn.startswith("ds_"):
        return "LDS"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vector memory"
    if mn.startswith("s_") and not mn.startswith(("s_barrier", "s_endpgm", "s_sleep", "s_set", "s_sendmsg", "s_trap")):
        return "SALU"
    return "other"


SCALAR_CLASSES = ("SALU", "branch", "s_waitcnt", "s_nop", "scalar memory", "LDS", "vector memory", "other")


def base(mn):
    return re.sub(r"_(e32|e64|dpp|sdwa)$", "", mn)


def blocks_of(body):
    """basic blocks [(label, first line, [(mnemonic, text)])] in listing order: a label starts one, a branch ends one (the code behind
    a conditional branch is a block of its own, named label+n)"""
    out, cur, n = [], ("entry", 0, []), 0
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            out.append(cur)
            cur, n = (m.group(1), i, []), 0
            continue
        t = l.split(";")[0].strip()
        if t and not t.startswith("."):
            if cur[2] and cur[2][-1][0].startswith(("s_branch", "s_cbranch")):
                out.append(cur)
                n += 1
                cur = ("%s+%d" % (cur[0].split("+")[0], n), i, [])
            cur[2].append((t.split()[0], t))
    out.append(cur)
    return out


def resources(lines, end):
    """the compiler's kernel-info comments after the function"""
    res = {}
    for l in lines[end:end + 40]:
        m = re.match(r"; (TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", l)
        if m:
            res[m.group(1)] = int(m.group(2))
    return res


def main():
    argv = sys.argv[1:]
    through = ["ds_write2"] if "--committing" in argv else []
    if "--momentum" in argv:
        through.append(r"ds_read2_b64 \S+ \S+ offset1:1$")
    while "--through" in argv:
        through.append(argv[argv.index("--through") + 1])
        del argv[argv.index("--through"):argv.index("--through") + 2]
    want = (1 << len(through)) - 1
    run_masked = "--momentum" in argv      # (an exec-masked region is run, not skipped: its s_cbranch_execz is never taken while a lane is in it)
    args = [a for a in argv if not a.startswith("--")]
    listing = compile_listing(args[0]) if "--compile" in sys.argv else args[0]
    lines = open(listing).read().split("\n")
    start = next(i for i, l in enumerate(lines) if args[1] in l and re.match(r"^[A-Za-z_][\w.]*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    name = body[0].split(":")[0]
    res = resources(lines, end)
    print(name)
    print("  vgpr %s  agpr %s  sgpr %s  scratch %s B/lane  static LDS %s B  occupancy %s" % tuple(
        res.get(k) for k in ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")))
    blocks = blocks_of(body)
    index = {b[0]: k for k, b in enumerate(blocks)}
    edges = [(k, index[t.split()[-1]], mn) for k, (_, _, ins) in enumerate(blocks) for mn, t in ins
             if mn.startswith(("s_branch", "s_cbranch")) and t.split()[-1] in index]
    # Innermost loops, as [(head, members)].  A backward branch closes a loop only if its target heads one: hipcc also lays a rarely
    # skipped stretch of a loop's body out of line, behind (or in front of) the rest, and jumps back into the body from there (the
    # certified loops' screened iteration).  Where the listing carries the compiler's loop comments the heads are the labels followed by
    # "This Inner Loop Header" and the members the blocks marked "in Loop: Header=<that label>", wherever they lie; without comments:
    # every innermost range closed by a backward branch, as before.
    heads = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m and any("This Inner Loop Header" in x for x in body[i:i + 3] if x is l or x.lstrip().startswith(";")):
            heads[m.group(1)] = {m.group(1)}
    for l in body:
        m = re.match(r"^(\.LBB\d+_\d+):.*in Loop: Header=(BB\d+_\d+) ", l)
        if m and ".L" + m.group(2) in heads:
            heads[".L" + m.group(2)].add(m.group(1))
    if heads:
        inner = sorted((index[h], sorted(k for k, blk in enumerate(blocks) if blk[0].split("+")[0] in names)) for h, names in heads.items())
    else:
        loops = sorted({(dst, src) for src, dst, _ in edges if dst <= src})
        inner = [(a, list(range(a, b + 1))) for a, b in loops if not any((c, d) != (a, b) and a <= c and d <= b for c, d in loops)]
    nvalu = [sum(1 for mn, _ in blk[2] if is_valu(mn)) for blk in blocks]
    for head, members in inner:
        a, b = members[0], members[-1]
        # the cheapest way through the body: from the head to a block that goes back to the head, along the body's edges (fall-through
        # or branch, forward or backward)
        inside = set(members)
        succ = {k: set() for k in members}
        for k in members:
            ins = blocks[k][2]
            if not (ins and ins[-1][0] == "s_branch") and k + 1 in inside:
                succ[k].add(k + 1)
        for src, dst, mn in edges:
            if src in inside and dst in inside and not (run_masked and mn == "s_cbranch_execz"):
                succ[src].add(dst)
        latches = [k for k in members if head in succ[k]]
        for k in members:
            succ[k].discard(head)
        # (--through RE: the cheapest path that executes an instruction matching RE -- the segment sums: 'permlane'; the state of the
        # search is the block and the set of REs met so far, as a bit mask)
        has = [sum(1 << j for j, rx in enumerate(through) if any(re.search(rx, t) for _, t in blk[2])) for blk in blocks]
        cost = {(head, has[head]): (nvalu[head], None)}
        changed = True
        while changed:      # (relaxed until nothing moves: the body's edges need not run forward)
            changed = False
            for k in members:
                for seen in range(want + 1):
                    if (k, seen) in cost:
                        for n in succ[k]:
                            st = (n, seen | has[n])
                            c = cost[(k, seen)][0] + nvalu[n]
                            if st not in cost or c < cost[st][0]:
                                cost[st] = (c, (k, seen))
                                changed = True
        ends = [(cost[(k, want)][0], k) for k in latches if (k, want) in cost]
        path, st = [], (min(ends)[1], want) if ends else None
        while st is not None:
            path.append(st[0])
            st = cost[st][1]
        hot = [(mn, t) for k in path for mn, t in blocks[k][2]]
        f64 = collections.Counter(base(mn) for mn, _ in hot if base(mn) in F64)
        dpp_mov = sum(1 for mn, t in hot if mn.startswith("v_mov_b32") and re.search(r"quad_perm|row_|wave_", t))
        dpp_op = sum(1 for mn, t in hot if is_valu(mn) and not mn.startswith("v_mov_b32") and re.search(r"quad_perm|row_", t))
        perm = sum(1 for mn, _ in hot if mn.startswith("v_permlane"))
        last = blocks[b + 1][1] if b + 1 < len(blocks) else len(body)
        print("  loop %s..%s (listing lines %d..%d): VALU %d in all, %d on the cheapest path | on it: %s, DPP moves %d, DPP-fused ops %d, "
              "permlanes %d" % (blocks[a][0], blocks[b][0], start + blocks[a][1] + 1, start + last, sum(nvalu[k] for k in members),
                                sum(1 for mn, _ in hot if is_valu(mn)), " ".join("%s %d" % (f, f64[f]) for f in F64), dpp_mov, dpp_op, perm))
        if "--mnemonics" in sys.argv:
            print("    on the path: " + ", ".join("%s %d" % kv for kv in sorted(collections.Counter(base(mn) for mn, _ in hot if is_valu(mn)).items())))
        if "--scalar" in sys.argv:
            cls = collections.Counter(scalar_class(mn) for mn, _ in hot if not is_valu(mn))
            print("    not VALU on the path: %d | %s" % (sum(cls.values()), ", ".join("%s %d" % (c, cls[c]) for c in SCALAR_CLASSES)))
            print("    SALU on the path: " + ", ".join("%s %d" % kv for kv in sorted(collections.Counter(mn for mn, _ in hot if scalar_class(mn) == "SALU" and not is_valu(mn)).items())))
        if "--blocks" in sys.argv:
            for k in members:
                br = [t for mn, t in blocks[k][2] if mn.startswith(("s_branch", "s_cbranch"))]
                print("    %-14s %-4s VALU %4d  %s" % (blocks[k][0], "path" if k in path else "", nvalu[k], "; ".join(br)))


if __name__ == "__main__":
    main()
