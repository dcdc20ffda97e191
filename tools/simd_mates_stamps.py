#!/usr/bin/env python3
"""When the two waves that share a SIMD start and finish, relative to each other, in one launch of the headline kernel (DESIGN.md
section 9 item 4, EXPERIMENTS.md "SIMD-mate waves").  Needs the diagnostic build, in which every wave of the loop-constants build
stamps its entry and exit (biconvex_admm_body.h: simd_stamp; the shipped library executes no stamp):

    BUNMPC_EXTRA_FLAGS=-DBMPC_SIMD_STAMPS BUNMPC_LIB_OUT=/tmp/libbunmpc_stamps.so python -m bunmpc_amd.build
    BUNMPC_LIB=/tmp/libbunmpc_stamps.so tools/simd_mates_stamps.py [--out FILE] [--batch 4096] [--warmup 5]

One stamped launch of the bench batch after the warm-up launches, then the table: which grid indices share a SIMD, which of the two
entered first, (younger's finish - older's finish) / kernel time, the share of kernel time with two, one and no live wave per SIMD,
kernel time over mean wave life, the in-kernel clock.  Then a lone wave of the same build: half the batch forced onto the two-waves
build (one wave per SIMD if the dispatcher spreads them: the stamps say), timed against the full batch.  `predictions()` holds what the
issue's model expects for each line; it is printed beside the measurement and was written before the first run."""
import argparse, ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

WORDS = 8      # per wave: [0] 100 MHz clock at entry, [1] HW_ID | XCC_ID << 32, [2] shader clock at entry, [3], [4] the clocks at exit


def simd_key(word):
    """(xcc, shader engine, shader array, CU, SIMD) of a stamp's id word as one integer, and the wave slot: HW_REG_HW_ID has the
    wave slot in bits 3:0, the SIMD in 5:4, the CU in 11:8, the shader array in 12, the shader engine in 15:13; XCC_ID is bits 3:0."""
    hw, xcc = word & 0xffffffff, (word >> 32) & 0xf
    return (xcc << 16) | (hw & 0xff30), hw & 0xf


def table(st):
    """the measurements of one stamped launch, from its [waves][8] words: a dict of numbers and small arrays"""
    st = np.asarray(st, dtype=np.uint64).reshape(-1, WORDS).astype(np.int64)
    t_in, t_out, c_in, c_out = st[:, 0], st[:, 3], st[:, 2], st[:, 4]
    key = np.array([simd_key(int(w))[0] for w in st[:, 1]])
    t0, t1 = t_in.min(), t_out.max()
    kernel = float(t1 - t0)
    life = (t_out - t_in).astype(float)
    out = {"waves": len(st), "kernel_us": kernel / 100.0, "kernel_over_mean_life": kernel / life.mean(),
           "life_min_mean_max_us": (float(life.min()) / 100.0, float(life.mean()) / 100.0, float(life.max()) / 100.0),
           "entry_spread_us": float(t_in.max() - t0) / 100.0,
           "clock_mhz": float(np.median((c_out - c_in) / np.maximum(t_out - t_in, 1))) * 100.0}
    groups = {}
    for w, k in enumerate(key):
        groups.setdefault(int(k), []).append(w)
    sizes = np.bincount([len(g) for g in groups.values()])
    out["simds"] = len(groups)
    out["waves_per_simd_hist"] = {n: int(c) for n, c in enumerate(sizes) if c}
    two = one = none = 0.0
    rel, gaps, first_is_lower, entry_gap, life_old, life_young = [], [], 0, [], [], []
    pairs = [g for g in groups.values() if len(g) == 2]
    for g in groups.values():
        iv = sorted((t_in[w], t_out[w]) for w in g)
        # time with >= 1 and >= 2 live waves (sweep; any number of waves on the SIMD)
        ev = sorted([(a, 1) for a, _ in iv] + [(b, -1) for _, b in iv])
        live, last, ge1, ge2 = 0, t0, 0.0, 0.0
        for t, d in ev:
            if live >= 1: ge1 += t - last
            if live >= 2: ge2 += t - last
            live, last = live + d, t
        two += ge2; one += ge1 - ge2; none += kernel - ge1
    for a, b in pairs:
        old, young = (a, b) if (t_in[a], a) <= (t_in[b], b) else (b, a)
        rel.append((t_out[young] - t_out[old]) / kernel)
        gaps.append(abs(a - b))
        first_is_lower += old < young
        entry_gap.append((t_in[young] - t_in[old]) / 100.0)
        life_old.append(life[old]); life_young.append(life[young])
    n = max(len(groups), 1)
    out["share_two_one_none"] = (float(two / n / kernel), float(one / n / kernel), float(none / n / kernel))
    if pairs:
        rel = np.array(rel)
        vals, cnt = np.unique(gaps, return_counts=True)
        top = np.argsort(-cnt)[:6]
        out["pairs"] = len(pairs)
        out["index_gap_top"] = [(int(vals[i]), int(cnt[i])) for i in top]
        out["older_is_lower_index"] = first_is_lower / len(pairs)
        out["entry_gap_us_median_max"] = (float(np.median(entry_gap)), float(np.max(entry_gap)))
        out["younger_minus_older_over_kernel"] = {"mean": float(rel.mean()), "mean_abs": float(np.abs(rel).mean()), "younger_later": float((rel > 0).mean()),
                                                  "pct_5_25_50_75_95": [float(x) for x in np.percentile(rel, [5, 25, 50, 75, 95])]}
        out["mean_life_older_younger_us"] = (float(np.mean(life_old)) / 100.0, float(np.mean(life_young)) / 100.0)
    return out


def predictions():
    """What the issue's model says, written before the first run.  The model: a wave costs max over its two problems of force
    iterations x 174 + motion iterations x 164, plus 2763 per ADMM iteration; a SIMD with two live waves delivers 2 units, with one
    1 / c1 units, c1 = 0.84 (a lone wave 2.30 ms against a pair 2.75 ms, an older build)."""
    return {
        "index_gap_top": "two guesses: adjacent grid indices (gap 1), or i and i + 1024 (gap 1024)",
        "older_is_lower_index": "1.0 if workgroups are dispatched in grid order",
        "younger_minus_older_over_kernel": "fair sharing: symmetric about 0, mean |.| about 0.03 (the mates' work differs by ~4.5 % of the mean, the "
                                           "remainder runs at the lone rate); the guide's rule (older unimpeded, younger the leftover): positive "
                                           "on nearly every SIMD, mean 0.3 or more",
        "share_two_one_none": "fair sharing: one live wave 0.03 .. 0.05 of kernel time, none about 0.08 (kernel 1.08 .. 1.11, mean SIMD 1.005 .. "
                              "1.011); the guide's rule: one live wave 0.3 or more (kernel 1.15 .. 1.23, mean SIMD 1.10 .. 1.13)",
        "kernel_over_mean_life": "fair sharing 1.08 .. 1.11 (slowest wave 13.8 % above the mean); the guide's rule 1.15 .. 1.23 against the paired mean",
        "clock_mhz": "2400 at the most (the part's peak engine clock); lower under a sustained fp64 load",
        "lone": "lone throughput / paired throughput about 0.6 (c1 = 0.84: t_pair / (2 t_lone) = 2.75 / 4.60)",
        "gate": "one-live share x (1 - lone / paired): fair sharing 0.04 x 0.4 = 0.016, below the gate of 0.02; the guide's rule 0.3 x 0.4 = 0.12",
    }


def show(title, tab, pred, put):
    put("== " + title)
    for k, v in tab.items():
        put("%-34s %s" % (k, v))
        if pred and k in pred:
            put("%-34s   predicted: %s" % ("", pred[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mate-balance", type=int, default=None, help="bmpc_set_simd_mate_balance(mode) before the stamped launches, where the library has it")
    args = ap.parse_args()
    import torch
    from bunmpc_amd import _lib, batch as bb, problems
    lib = _lib.lib()
    try:
        set_buffer = lib.bmpc_simd_stamps_buffer
    except AttributeError:
        sys.exit("this library executes no stamp: build it with BUNMPC_EXTRA_FLAGS=-DBMPC_SIMD_STAMPS and name it in BUNMPC_LIB")
    set_buffer.argtypes, set_buffer.restype = [ctypes.c_void_p], None
    if args.mate_balance is not None:
        lib.bmpc_set_simd_mate_balance.argtypes, lib.bmpc_set_simd_mate_balance.restype = [ctypes.c_int], ctypes.c_int
        lib.bmpc_set_simd_mate_balance(args.mate_balance)
    lines = []

    def put(s):
        print(s, flush=True)
        lines.append(s)

    def timed(db, n=20):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record(); db.solve(); b.record()
        torch.cuda.synchronize()
        ms = np.array([a.elapsed_time(b) for a, b in ev])
        return float(np.median(ms)), float(ms.min()), float(ms.max())

    def stamped(db, B):
        buf = torch.zeros(((B + 1) // 2 + 8) * WORDS, dtype=torch.int64, device="cuda")
        set_buffer(buf.data_ptr())
        db.solve()
        torch.cuda.synchronize()
        set_buffer(None)
        words = buf.cpu().numpy()[: (B + 1) // 2 * WORDS]
        if not (words.reshape(-1, WORDS)[:, [0, 3]] != 0).all():      # (only the loop-constants build stamps)
            sys.exit("the stamped launch (%s) left waves without stamps: not the loop-constants build?" % lib.bmpc_biconvex_last_kernel_name().decode())
        return words

    pred = predictions()
    B = args.batch
    put("# tools/simd_mates_stamps.py: solo12_trot, B = %d, 10 ADMM iterations, %d warm-up launches, one stamped launch; %s" % (B, args.warmup, torch.cuda.get_device_name(0)))
    db = bb.DeviceBatch(problems.make_batch("solo12_trot", B), num_iters=10)
    for _ in range(args.warmup):
        db.solve()
    torch.cuda.synchronize()
    raw = stamped(db, B)
    if args.out:      # (the raw words and the solve's counts beside the table, for another look without another run)
        np.save(args.out + ".stamps.npy", raw)
        np.save(args.out + ".stats.npy", db.results()["stats"])
    full = table(raw)
    show("full batch, two waves per SIMD", full, pred, put)
    t_pair = timed(db)
    put("%-34s median %.4f ms (min %.4f, max %.4f; 20 launches, device events, stamps off)" % ("launch time, B = %d" % B, *t_pair))
    del db
    # a lone wave of the same build: half the batch, forced onto the two-waves build
    old = lib.bmpc_set_two_waves_per_simd(1)
    try:
        dh = bb.DeviceBatch(problems.make_batch("solo12_trot", B // 2), num_iters=10)
        for _ in range(args.warmup):
            dh.solve()
        torch.cuda.synchronize()
        half = table(stamped(dh, B // 2))
        show("half batch, forced onto the two-waves build (lone waves where the histogram says 1)", half, None, put)
        t_lone = timed(dh)
        put("%-34s median %.4f ms (min %.4f, max %.4f)" % ("launch time, B = %d" % (B // 2), *t_lone))
    finally:
        lib.bmpc_set_two_waves_per_simd(old)
    put("== lone wave against a pair, and the gate")
    put("%-34s   predicted: %s" % ("", pred["lone"]))
    # by launch times (the half batch holds the full batch's first half: its slowest wave need not be the full batch's) and by mean wave life
    r_time = t_pair[0] / (2.0 * t_lone[0])
    r_life = full["life_min_mean_max_us"][1] / (2.0 * half["life_min_mean_max_us"][1])
    put("%-34s by launch time %.3f, by mean wave life %.3f" % ("lone / paired throughput", r_time, r_life))
    one = full["share_two_one_none"][1]
    put("%-34s   predicted: %s" % ("", pred["gate"]))
    for name, r in (("launch time", r_time), ("mean wave life", r_life)):
        put("%-34s %.4f x (1 - %.3f) = %.4f of the launch (gate: 0.02)" % ("gate, lone rate by " + name, one, r, one * (1.0 - r)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
