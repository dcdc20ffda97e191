"""The priority rule of the headline kernel's SIMD-mate waves (biconvex_admm_body.h: MATES) as a small model:
the rule itself, and two waves sharing one SIMD's issue slots.

A wave's solve is a sequence of phases, each a cost in issue slots.  At the head of its n-th phase (counted from 1) a wave publishes n
in its mailbox word, reads its mate's word m and sets its priority by `rule`; behind its last phase it publishes DONE.  The SIMD delivers

    both waves live, different priorities    hi to the wave of the higher priority, lo to the other
    both live, equal priorities              the same split with the OLDER wave (wave 0) as the favoured one -- or, fair=True, 1 each
    one wave live                            lone

with hi + lo = 2, the pair's throughput.  profiles/simd_mates_step0.txt: a lone wave delivers 0.65 .. 0.69 of a pair's throughput, lone =
1.34; at equal priority the older wave lives 1620 us against the younger's 2244 us, 0.722 of it, and with equal work that ratio is
1 / (1 + (hi - lo) / lone): hi - lo = 0.52, hi = 1.26, lo = 0.74 -- the older wave runs close to the lone rate, the younger on the rest."""
import numpy as np

DONE = 0x7fffffff
HI, LO, LONE = 1.26, 0.74, 1.34


def rule(n, m):
    """the priority a wave sets at the head of its phase n on reading m from its mate: 1 where the mate is level or ahead and still
    solving, else 0 (the mate is behind, has published nothing yet, or has finished)"""
    return 1 if (m >= n and m != DONE) else 0


def simulate(costs0, costs1, rule_on=True, fair=False, publishes=(True, True), hi=HI, lo=LO, lone=LONE):
    """finish times (t0, t1) of wave 0 (the older) and wave 1 with these phase costs; publishes[w] False: wave w never writes its word"""
    costs = [np.asarray(costs0, float), np.asarray(costs1, float)]
    word, prio, phase, left, done_at = [0, 0], [0, 0], [0, 0], [0.0, 0.0], [None, None]
    t = 0.0

    def boundary(w):
        """wave w enters its next phase, or finishes"""
        n = phase[w] + 1
        if n > len(costs[w]):
            done_at[w] = t
            if publishes[w]:
                word[w] = DONE
            return
        phase[w], left[w] = n, costs[w][n - 1]
        if publishes[w]:
            word[w] = n
        if rule_on:
            prio[w] = rule(n, word[1 - w])

    boundary(0)
    boundary(1)
    while done_at[0] is None or done_at[1] is None:
        live = [w for w in (0, 1) if done_at[w] is None]
        if len(live) == 1:
            rate = {live[0]: lone}
        elif prio[0] != prio[1]:
            fav = 0 if prio[0] > prio[1] else 1
            rate = {fav: hi, 1 - fav: lo}
        else:
            rate = {0: 1.0, 1: 1.0} if fair else {0: hi, 1: lo}
        dt = min(left[w] / rate[w] for w in live)
        t += dt
        for w in live:
            left[w] -= dt * rate[w]
        for w in live:
            if left[w] <= 1e-9 * max(1.0, costs[w].max(initial=1.0)):
                boundary(w)
    return done_at[0], done_at[1]


def wave_phase_costs(it_f, it_x, valu_f=174.0, valu_x=164.0, per_iter=2763.0):
    """[waves][2 num_iters] phase costs of consecutive problem pairs from the FISTA iterations per phase, it_f and it_x [B][num_iters]:
    a wave pays the larger count of its two problems, the rest of the ADMM iteration rides on the motion phase"""
    f = np.maximum(it_f[0::2], it_f[1::2]) * valu_f
    x = np.maximum(it_x[0::2], it_x[1::2]) * valu_x + per_iter
    return np.stack([f, x], axis=2).reshape(f.shape[0], -1)
