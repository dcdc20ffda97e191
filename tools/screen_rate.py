#!/usr/bin/env python3
"""How often the lane-local screen of the benchmark kernel's certified FISTA loops settles an iteration (biconvex_lanes.h:
screen_theta; biconvex_admm_body.h: `theta`) -- the numpy restatement, on oracle/oracle_np.py.

In a certified loop an iteration needs the squared step |d|^2 = sum of the lanes' (knots') partials for two decisions only: "below the
floor?" (hand the phase to the tested loop) and "below tol^2?" (exit).  The partials are non-negative and fl(a + b) >= max(a, b) for
a, b >= 0, so the sum in any order is at least the largest partial: one lane with a partial above

    theta = max(max(tol^2, floor2) (1 + 2^-40), 2^-1000)

settles both decisions ("no") and keeps the sum clear of the 1e-14 band around tol^2 in which the reference's sqrt form is evaluated.
A wave-iteration is screened when every problem of the wave that still iterates has such a lane; then the wave takes no sum at all.

    python tools/screen_rate.py [--config solo12_trot] [--B 24] [--waves 12] [--num-iters 10] [--per-wave 2]
                                [--terms force=2 motion=3,5 ...] [--quad]

solves the problems of `waves` waves spread evenly over the config's batch of B (a wave: per-wave consecutive problems, as the kernel
takes them) with oracle_np, every FISTA step recorded knot by knot, and prints, per step, the wave-iterations and the share of them
the screen settles.  Every phase is
counted as certified (on the benchmark's trot batch every phase is: tools/certify_rate.py).  The floor is restated from the oracle's
whole b - P (the kernel leaves out the x_init rows of the motion step: a slightly lower floor there); on the benchmark's settings
tol^2 = 1e-10 is far above it and sets theta alone.

--terms: the two-stage screen (biconvex_admm_body.h: kScreenTermsX, kScreenTermsF).  Stage 1 asks the same question of the sum of a FEW
of the knot's squares -- the components named, indices into the knot's 9 motion or 3 E force variables; a subset's sum is at most the
whole, so a hit is as sound -- and only a miss computes the whole partial.  Per step and set of terms given (any number of
force=... / motion=... items): the share of wave-iterations stage 1 settles and the expected vector instructions per iteration,
2 k + P(miss) (2 n + 1) for k terms of n (a subtraction and an fma per term, one compare more on a miss) -- against 2 n for one stage."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ETA = 2.0 ** -6                                      # biconvex_admm_body.h: kCertEta
CERT_FLOOR = 2.0 * 25.0 / (ETA * ETA) * 2.0 ** -80   # kCertFloor


def theta(tol2, floor2):
    """screen_theta (biconvex_lanes.h); fmax semantics: a NaN operand is dropped"""
    return np.fmax(np.fmax(tol2, floor2) * (1.0 + 2.0 ** -40), 2.0 ** -1000)


def butterfly_sum32(p):
    """seg_sum<32> (biconvex_lanes.h) on [..., 32] partials: quad xor 1, quad xor 2, half-row mirror, row mirror, 16-lane swap --
    the kernel's order of additions, hence its bits; every lane ends with the same value, returned as [...]"""
    v = np.array(p, np.float64)
    lane = np.arange(32)
    for src in (lane ^ 1, lane ^ 2, (lane & ~7) | (7 - (lane & 7)), (lane & ~15) | (15 - (lane & 15)), lane ^ 16):
        with np.errstate(invalid="ignore", over="ignore"):
            v = v + v[..., src]
    return v[..., 0]


def verdicts(S, tol2, floor2):
    """the three fp64 questions a certified iteration asks of the summed step S: below the floor, done, inside the edge band"""
    with np.errstate(invalid="ignore", over="ignore"):
        return S < floor2, S < tol2, np.abs(S - tol2) <= 1e-14 * tol2


def floor2_of(bPk, x0, L, rho):
    """cert_floor (biconvex_admm_body.h) for one problem: (|bPk|^2 + (T / rho)|x_0|^2) kCertFloor rho / (L/2), T = (L/2)(1 - eta)"""
    Lh = 0.5 * L
    return (bPk @ bPk + (Lh * (1.0 - ETA) / rho) * (x0 @ x0)) * CERT_FLOOR * (rho / Lh)


def record_solve(b, i, num_iters=10, maxit=150, tol=1e-5):
    """problem i of the batch through oracle_np.biconvex_solve with every FISTA step recorded: returns {"force": [...], "motion": [...]},
    one (squares [iterations][knots][components], floor2) per phase -- squares[k][t] sums to knot t's share of |d|^2 in iteration k"""
    from oracle import oracle_np as on
    width = {True: 3 * b.E, False: 9}      # keyed by "the force phase": the solver with a projection
    phases = {True: [], False: []}

    class Recorder(on.Fista):
        def step(self, p, y):
            y1, G = super().step(p, y)
            d = (y1 - y).reshape(-1, width[self.projection is not None])
            self._rows.append(d * d)
            return y1, G

        def optimize(self, p, maxit, tol):
            self._rows = []
            fl = floor2_of(p.bPk, p.x, self.L, p.rho)
            its = super().optimize(p, maxit, tol)
            phases[self.projection is not None].append((np.array(self._rows), fl))
            return its

    sb = 0 if b.W_X.shape[0] == 1 else i
    Qx, qx = on.create_cost_X(b.W_X[sb], b.W_X_ter[sb], b.X_ter[i], b.X_nom[i])
    lbx, ubx = on.create_bound_constraints(b.cnt_plan[i], b.bounds[0 if b.bounds.shape[0] == 1 else i])
    Qf = b.W_F[0 if b.W_F.shape[0] == 1 else i]
    X0, F0, P0 = b.warm_start()
    on.biconvex_solve(b.cnt_plan[i], b.dt[i], b.m, b.x_init[i], Qx, qx, Qf, lbx, ubx, X0[i], F0[i], P0[i], rho=b.rho,
                      num_iters=num_iters, maxit=maxit, tol=tol, mu=getattr(b, "mu", 1.0), fista=Recorder)
    return {"force": phases[True], "motion": phases[False]}


def quad_settles(row, th):
    """does the quad stage settle a problem?  The knots' partials [knots] on lanes 0 .. (knot t on lane t, the lanes past the last knot
    hold zeros), through the numpy model the kernel's helpers are held to bit for bit (tests/quad_screen_np.py: the fp32 sum of each
    aligned group of four lanes against float(theta (1 + 2^-20)))"""
    from tests import quad_screen_np
    v = np.zeros(32)
    v[:len(row)] = row
    return bool(np.any(quad_screen_np.quad_screen(v, th)))


def wave_rate(records, which, tol=1e-5, terms=None, quad=False):
    """(screened, total) wave-iterations of one wave: records = [record_solve(...)] of its problems.  Per phase the wave runs as many
    iterations as its longest problem; theta takes the largest floor of the problems that run the phase; an iteration is screened
    when every problem still iterating has a knot above theta.  terms: the components whose squares are summed (default: all).
    quad: a problem also counts as settled when the quad stage settles it (quad_settles)."""
    hit = total = 0
    cols = slice(None) if terms is None else list(terms)
    for k in range(max(len(r[which]) for r in records)):
        ph = [r[which][k] for r in records if k < len(r[which])]
        th = theta(tol * tol, max(fl for _, fl in ph))
        for it in range(max(len(p) for p, _ in ph)):
            live = [p[it][:, cols].sum(1) for p, _ in ph if it < len(p)]
            hit += all(bool(np.any(row > th)) or (quad and quad_settles(row, th)) for row in live)
            total += 1
    return hit, total


def rates_of(recs, which, per_wave=2, tol=1e-5, terms=None, quad=False):
    """(screened, total) wave-iterations of one step over recorded solves taken per_wave at a time"""
    hit = total = 0
    for w in range(0, len(recs), per_wave):
        h, n = wave_rate(recs[w:w + per_wave], which, tol, terms, quad)
        hit, total = hit + h, total + n
    return hit, total


def rates(b, indices, per_wave=2, num_iters=10, maxit=150, tol=1e-5):
    recs = [record_solve(b, i, num_iters, maxit, tol) for i in indices]
    return {which: rates_of(recs, which, per_wave, tol) for which in ("force", "motion")}


def parse_terms(items):
    """["force=2", "motion=3,5", "force=2,5"] -> [("force", (2,)), ("motion", (3, 5)), ("force", (2, 5))]"""
    out = []
    for it in items:
        which, _, idx = it.partition("=")
        if which not in ("force", "motion") or not idx:
            raise ValueError("--terms takes force=i,j,... or motion=i,j,...: %r" % it)
        out.append((which, tuple(int(x) for x in idx.split(","))))
    return out


def stage_cost(k, n, p_hit):
    """expected vector instructions of the two-stage screen per iteration: k of n terms first, the whole chain and a compare on a miss"""
    return 2 * k + (1.0 - p_hit) * (2 * n + 1)


def main():
    from bunmpc_amd import problems
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", default="solo12_trot")
    ap.add_argument("--B", type=int, default=24)
    ap.add_argument("--waves", type=int, default=0, help="waves sampled, spread evenly over the batch (default: all)")
    ap.add_argument("--num-iters", type=int, default=10)
    ap.add_argument("--per-wave", type=int, default=2)
    ap.add_argument("--terms", nargs="+", default=[], metavar="STEP=I,J", help="stage-1 term sets of the two-stage screen to rate, e.g. force=2 motion=3,5")
    ap.add_argument("--quad", action="store_true", help="also rate a stage on the fp32 sum of the lane's DPP quad (knot t on lane t: the four-feet layout)")
    args = ap.parse_args()
    term_sets = parse_terms(args.terms)
    b = problems.make_batch(args.config, args.B)
    n_waves = -(-args.B // args.per_wave)
    picked = sorted({int(w) for w in np.linspace(0, n_waves - 1, min(args.waves or n_waves, n_waves))})
    idx = [i for w in picked for i in range(w * args.per_wave, min((w + 1) * args.per_wave, args.B))]
    recs = [record_solve(b, i, args.num_iters) for i in idx]      # (a last wave with fewer problems comes last: the pairing holds)
    for which in ("force", "motion"):
        hit, total = rates_of(recs, which, args.per_wave)
        print("%-12s %-6s %d problems in waves of %d: %6d wave-iterations, %6d screened (%.1f %%), %.1f per wave"
              % (args.config, which, len(idx), args.per_wave, total, hit, 100.0 * hit / max(total, 1), total / max(1, -(-len(idx) // args.per_wave))))
    if args.quad:      # a further stage between the lane's whole partial and the segment sum: the partial summed over the lane's DPP quad.
        # Knot t on lane t: the motion loop's layout and the four-feet force loop's.  The force loop with two feet per lane sums quads of
        # UNITS (per-unit partials of up to two feet, 26 .. 28 lanes): its rate is not this one, and is not modelled here.
        for which in ("force", "motion"):
            hit, total = rates_of(recs, which, args.per_wave)
            hq, _ = rates_of(recs, which, args.per_wave, quad=True)
            print("%-12s %-6s quad stage: %6d of the %6d unsettled wave-iterations settled; unsettled share %.1f %% -> %.1f %%"
                  % (args.config, which, hq - hit, total - hit, 100.0 * (total - hit) / max(total, 1), 100.0 * (total - hq) / max(total, 1)))
    width = {"force": 3 * b.E, "motion": 9}
    for which, terms in term_sets:
        hit, total = rates_of(recs, which, args.per_wave, terms=terms)
        print("%-12s %-6s stage 1 on terms %-12s %6d of %6d wave-iterations settled (%.1f %%), expected cost %.2f instructions (one stage: %d)"
              % (args.config, which, ",".join(map(str, terms)), hit, total, 100.0 * hit / max(total, 1),
                 stage_cost(len(terms), width[which], hit / max(total, 1)), 2 * width[which]))


if __name__ == "__main__":
    main()
