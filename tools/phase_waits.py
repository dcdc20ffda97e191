#!/usr/bin/env python3
"""Memory operations and waits of one kernel in a hipcc -S listing, per loop-nest level: where a kernel waits for memory OUTSIDE its hot
loops -- the phase prologues and the epilogue of the headline kernel's ADMM loop, which run ten times per solve.

    python tools/phase_waits.py LISTING.s KERNEL_SUBSTRING [--level N]
    python tools/phase_waits.py --compile admm_diag_f64_e4 KERNEL_SUBSTRING [--level N]
        (--compile: device code of that job of bunmpc_amd/build.py, with its flags, as tools/loop_valu.py does)

Blocks are the compiler's own: a label `.LBB<f>_<n>:` or a fall-through comment `; %bb.<n>:` starts one, and its comment says where it
lies: `in Loop: Header=BB<f>_<h> Depth=<d>` (a block of that loop's body proper, not of a loop nested in it) or `This [Inner] Loop
Header: Depth=<d>` (the head of a loop of its own).  Per level d (0: outside every loop) and per loop the tool reports

    blocks, instructions, VALU, scratch loads / stores, global loads / stores, LDS instructions, waits on vmcnt, waits on lgkmcnt

and the MASKED SINGLE-READ BLOCKS: blocks entered behind `s_and_saveexec` (the block in front ends with it, or with it and an
`s_cbranch_execz`) whose only memory operation, scratch reloads aside, is ONE LDS read or ONE global load.  Such a block is what hipcc
makes of `ok ? array[l] : 0` with a lane predicate: one element, its own address reload, its own wait -- a dependent round trip that
nothing overlaps.  A batch read unconditionally with a select behind it has none of them.

Then the memseq string (tools/memseq.py: L global load, s global store, r / p scratch load / store, W a wait on vmcnt, d a run of LDS
instructions, w a wait on lgkmcnt alone) of the blocks of level --level (default 1: the ADMM loop's body), in listing order, a `/`
where blocks of another level lie between.  `rW` in front of a `d` is an address reloaded from scratch memory; an `rW` behind a run of
L waits for the whole run."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ("blocks", "instr", "valu", "scratch_ld", "scratch_st", "global_ld", "global_st", "lds", "wait_vm", "wait_lgkm", "masked_single_reads")


def compile_listing(job):
    sys.path.insert(0, ROOT)
    from bunmpc_amd import build
    out = os.path.join(tempfile.mkdtemp(), job + ".s")
    cmd = build.compile_cmd(build.job(job)) + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"), "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out


def kernel_body(lines, name):
    """the lines of the first function whose symbol holds `name`, label line included, up to its .Lfunc_end"""
    start = next(i for i, l in enumerate(lines) if name in l and re.match(r"^[A-Za-z_][\w.$]*:", l))
    end = next((i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end")), len(lines))
    return lines[start:end]


def is_valu(mn):
    return mn.startswith("v_")


def blocks_of(body):
    """[dict(label, loop, depth, ins=[(mnemonic, text)])] in listing order.  loop: the header label (without .L) of the loop whose
    body the block belongs to, None outside every loop; a loop's head belongs to its own loop."""
    out = []
    cur = dict(label="entry", loop=None, depth=0, ins=[])
    k = 0
    while k < len(body):
        l = body[k]
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", l) or re.match(r"^; (%bb\.\d+):(.*)$", l)
        if m:
            out.append(cur)
            label, rest = m.group(1), m.group(2)
            cur = dict(label=label, loop=None, depth=0, ins=[])
            # the comment on the label's line and on the comment-only lines under it
            notes = [rest]
            while k + 1 < len(body) and re.match(r"^\s+;", body[k + 1]):
                k += 1
                notes.append(body[k])
            for n in notes:
                h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", n)
                if h:
                    cur["loop"], cur["depth"] = h.group(1), int(h.group(2))
                h = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", n)
                if h:
                    cur["loop"], cur["depth"] = label[2:] if label.startswith(".L") else label, int(h.group(1))
            k += 1
            continue
        t = l.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            cur["ins"].append((t.split()[0], t))
        k += 1
    out.append(cur)
    return out


def is_wait(t, counter):
    return t.startswith("s_waitcnt") and counter in t


def counts(block):
    c = dict.fromkeys(COLUMNS, 0)
    c["blocks"] = 1
    for mn, t in block["ins"]:
        c["instr"] += 1
        c["valu"] += is_valu(mn)
        c["scratch_ld"] += mn.startswith("scratch_load")
        c["scratch_st"] += mn.startswith("scratch_store")
        c["global_ld"] += mn.startswith(("global_load", "flat_load"))
        c["global_st"] += mn.startswith(("global_store", "flat_store"))
        c["lds"] += mn.startswith("ds_")
        c["wait_vm"] += is_wait(t, "vmcnt")
        c["wait_lgkm"] += is_wait(t, "lgkmcnt")
    return c


def enters_masked(prev):
    """does the block behind `prev` run under an exec mask that `prev` has just narrowed?"""
    ins = [mn for mn, _ in prev["ins"]]
    while ins and (ins[-1] == "s_cbranch_execz" or ins[-1].startswith(("v_readlane", "v_mov", "s_mov", "s_nop"))):
        ins.pop()
    return bool(ins) and ins[-1].startswith("s_and_saveexec")


def is_masked_single_read(prev, block):
    if prev is None or not enters_masked(prev):
        return False
    mem = [mn for mn, _ in block["ins"] if mn.startswith(("ds_", "global_", "flat_", "buffer_"))]
    return len(mem) == 1 and mem[0].startswith(("ds_read", "global_load", "flat_load"))


def analyse(body):
    """(per level, per loop, blocks): {depth: counts}, {(depth, loop): counts}, the blocks with their own counts under 'c'"""
    blocks = blocks_of(body)
    per_level, per_loop = collections.OrderedDict(), collections.OrderedDict()
    prev = None
    for b in blocks:
        c = counts(b)
        c["masked_single_reads"] = int(is_masked_single_read(prev, b))
        b["c"] = c
        for table, key in ((per_level, b["depth"]), (per_loop, (b["depth"], b["loop"]))):
            acc = table.setdefault(key, dict.fromkeys(COLUMNS, 0))
            for k in COLUMNS:
                acc[k] += c[k]
        prev = b
    return per_level, per_loop, blocks


def memseq(blocks, level):
    """the order of memory operations and waits of the blocks of one level, `/` where other levels lie between"""
    seq, gap = [], False

    def put(c):
        nonlocal gap
        if gap and seq:
            seq.append("/")
        gap = False
        seq.append(c)

    for b in blocks:
        if b["depth"] != level:
            gap = True
            continue
        for mn, t in b["ins"]:
            if is_wait(t, "vmcnt"):
                put("W")
            elif is_wait(t, "lgkmcnt"):
                put("w")
            elif mn.startswith(("global_load", "flat_load")):
                put("L")
            elif mn.startswith(("global_store", "flat_store")):
                put("s")
            elif mn.startswith("scratch_load"):
                put("r")
            elif mn.startswith("scratch_store"):
                put("p")
            elif mn.startswith("ds_") and (gap or not seq or seq[-1] != "d"):
                put("d")
    return "".join(seq)


def main():
    argv = sys.argv[1:]
    level = 1
    if "--level" in argv:
        level = int(argv[argv.index("--level") + 1])
        del argv[argv.index("--level"):argv.index("--level") + 2]
    args = [a for a in argv if not a.startswith("--")]
    listing = compile_listing(args[0]) if "--compile" in argv else args[0]
    body = kernel_body(open(listing).read().split("\n"), args[1])
    per_level, per_loop, blocks = analyse(body)
    print(body[0].split(":")[0])
    head = "%-22s" + " %7s" * len(COLUMNS)
    short = ("blocks", "instr", "VALU", "scr ld", "scr st", "glb ld", "glb st", "LDS", "W vm", "W lgkm", "masked1")
    print(head % (("level / loop",) + short))
    for d in sorted(per_level):
        print(head % (("level %d" % d,) + tuple(per_level[d][k] for k in COLUMNS)))
        for (dd, loop), c in per_loop.items():
            if dd == d and loop is not None:
                print(head % (("  loop %s" % loop,) + tuple(c[k] for k in COLUMNS)))
    print("masked single-read blocks (masked1) at level %d: %d" % (level, per_level.get(level, dict.fromkeys(COLUMNS, 0))["masked_single_reads"]))
    print("memseq of level %d:" % level)
    print(memseq(blocks, level))


if __name__ == "__main__":
    main()
