import contextlib

import numpy as np
import pytest

from oracle import oracle_np


@contextlib.contextmanager
def knob_setter():
    """set_(setter name, value), callable many times: each call is a bunmpc_amd._lib.knobs block that stays open until this one ends, so
    everything is restored in reverse order.  A fixture with presets of its own sets them inside this block and yields set_."""
    from bunmpc_amd import _lib      # here, not at import: the tools that take rel_l2 and the envelopes from this module read no header
    keyword = {setter: k for k, setter in _lib.KNOBS.items()}

    def set_(name, value):
        if name not in keyword:
            raise TypeError("%s is not the setter of a dispatch knob (bunmpc_amd._lib.KNOBS)" % name)
        stack.enter_context(_lib.knobs(**{keyword[name]: value}))
    with contextlib.ExitStack() as stack:
        yield set_


@pytest.fixture
def knobs():
    """sets dispatch knobs for one test and restores every one of them afterwards: knobs("bmpc_set_two_waves_per_simd", 1)"""
    with knob_setter() as set_:
        yield set_


def launch_record(hiplib):
    """(kernel name, lanes per problem, waves per SIMD) of the last centroidal launch"""
    return hiplib.bmpc_biconvex_last_kernel_name().decode(), hiplib.bmpc_biconvex_last_lanes_per_problem(), hiplib.bmpc_biconvex_last_waves_per_simd()


def rel_l2(a, b):
    """relative L2 error of a against reference b (per problem when 2-D)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if a.ndim == 1:
        return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-300)


# ---- the envelope the GPU is held to where the reference algorithm itself is chaotic --------------------------
# Where the force FISTA sits on the expansive branch of the reference's "SoC" projection, rounding-order differences grow
# ~x1.12 per iteration and ANY two faithful implementations drift apart.  The three CPU restatements (strict C, matrix-free C,
# numpy twin) measure that drift on the very problems under test; the GPU, one more implementation with its own summation
# order, must stay within K_SPREAD times the largest pairwise distance among them -- and within north_star's 1e-5 wherever
# they agree.  K_SPREAD = 10: measured on the MI355X (tools/calibrate_parity.py, gpurun_out log of round 2) the ratio
# GPU-distance / CPU-spread over all chaotic problems of these tests has median 0.3-1.0 and maximum 2.7.
TOL_FP64 = 1e-5
K_SPREAD = 10.0


# ---- the CPU restatement of one problem, and the per-problem check of a kernel against it -------------------------------------
MAPPINGS = [(3, 16), (15, 16), (20, 21), (20, 32), (31, 32), (63, 64)]      # (H, lanes per problem) of the cost-shape kernels
LX = np.array([2.25e6, 1e4, 1e5, 3e5, 2.25e6, 5e4])      # step constants of six warm problems that force retries in both FISTA loops
LF = np.array([506.25, 10.0, 50.0, 506.25, 20.0, 100.0])


def problem_args(b, i, raw, warm=None, x_init=None):
    """the positional block of oracle_np.biconvex_solve and of the C oracle's biconvex_solve for problem i of batch b: raw[k][i] its
    cost and bound arrays (Qx, qx, Qf, lbx, ubx), warm = (X, F, P) of the batch or None for b.warm_start(); x_init: in place of
    b.x_init[i] (a cold start then begins at X = tile(x_init))"""
    X0, F0, P0 = b.warm_start() if warm is None else warm
    X = X0[i] if warm is not None or x_init is None else np.tile(x_init, b.H + 1)
    return (b.cnt_plan[i], b.dt[i], b.m, b.x_init[i] if x_init is None else x_init, raw["Qx"][i], raw["qx"][i], raw["Qf"][i],
            raw["lbx"][i], raw["ubx"][i], X, F0[i], P0[i])


def restatement(b, i, raw, iters, warm=None, L_x=2.25e6, L_f=506.25, x_init=None, qf=None, mu=None, problem=oracle_np.Problem,
                projection=oracle_np.soc_projection):
    """problem i of batch b through oracle_np.biconvex_solve, cold or from warm = (X, F, P); mu: in place of b.mu; problem and
    projection: the seams of oracle_np.biconvex_solve (a cost shape's ProblemData, a cone's projection)"""
    return oracle_np.biconvex_solve(*problem_args(b, i, raw, warm, x_init), L_x=L_x, L_f=L_f, rho=b.rho, num_iters=iters,
                                    mu=b.mu if mu is None else mu, qf=qf, problem=problem, projection=projection)


def assert_matches_twin(got, twins, spread_of=None, tol=TOL_FP64, keys="XFP", may_skip=0, disagree=None, tag=""):
    """The batch result `got` of a kernel against twins[i], the CPU restatement of problem i: the counts and both step constants equal,
    rel_l2 of every array of `keys` below the bound -- tol, or max(tol, K_SPREAD x the distance in X and F of spread_of[i], a second CPU
    run of the same problem, from twins[i]).  disagree: a second CPU run per problem whose counts must equal the twin's; a problem
    where they differ is left out and printed, and more than may_skip of them fail.  Prints what it compares; returns the twins'
    retries (both loops) over the problems compared."""
    retries, skipped = 0, []
    for i, r in enumerate(twins):
        if disagree is not None and not np.array_equal(r["stats"], disagree[i]["stats"]):
            print("LEFT OUT", tag, "problem", i, "CPU orders disagree:", r["stats"].tolist(), disagree[i]["stats"].tolist())
            skipped.append(i)
            continue
        bound = tol
        if spread_of is not None:
            bound = max(tol, K_SPREAD * max(rel_l2(spread_of[i][k], r[k]) for k in "XF"))
        err = {k: rel_l2(got[k][i], r[k]) for k in keys}
        print(tag, i, "stats", np.asarray(got["stats"][i]).tolist(), r["stats"].tolist(), "L", got["L_x"][i], got["L_f"][i], "err", err, "bound", bound)
        assert np.array_equal(got["stats"][i], r["stats"]), i
        assert got["L_x"][i] == r["L_x"] and got["L_f"][i] == r["L_f"], i
        for k in keys:
            assert err[k] < bound, (i, k, err[k], bound)
        retries += r["stats"][3] + r["stats"][4]
    assert len(skipped) <= may_skip, skipped
    return retries


def cpu_spread(b, iters, oracle, with_numpy=True, **kw):
    """strict C solution of batch b and, per problem, the largest pairwise rel-L2 distance (X and F) among the CPU restatements"""
    ref = oracle.solve_batch(b, num_iters=iters, **kw)
    fast = oracle.solve_batch(b, num_iters=iters, fast=True, **kw)
    s = np.maximum(rel_l2(fast["X"], ref["X"]), rel_l2(fast["F"], ref["F"]))
    if with_numpy:
        for i in range(b.B):
            rn = oracle_np.biconvex_solve(*problem_args(b, i, ref), rho=b.rho, num_iters=iters, mu=b.mu,
                                          **{k: v for k, v in kw.items() if k in ("maxit", "tol", "exit_tol")})
            s[i] = max(s[i], rel_l2(rn["X"], ref["X"][i]), rel_l2(rn["F"], ref["F"][i]), rel_l2(rn["X"], fast["X"][i]), rel_l2(rn["F"], fast["F"][i]))
    return ref, s


def within_envelope(got, ref, spread):
    """per problem: max(rel-L2 X, rel-L2 F) of the GPU result against the strict C solution, and the bound it must meet"""
    e = np.maximum(rel_l2(got["X"], ref["X"]), rel_l2(got["F"], ref["F"]))
    return e, np.maximum(TOL_FP64, K_SPREAD * spread)


# ---- prefix parity + per-problem CPU ensembles ----------------------------------------------------------
# What the GPU is held to on a problem of the chaotic regime, replacing the population-wide envelope of round 3:
#  (a) PREFIX PARITY.  The strict C oracle, the matrix-free C variant and N_MEMBERS one-ulp perturbations of x_init of each
#      (an ensemble of 2 + 2 N_MEMBERS CPU runs of the reference algorithm on "the same" problem) leave, per ADMM iteration,
#      the dynamics violation ||A_f X - b_f|| (biconvex.cpp:98-104) and the running FISTA iteration / retry counts.  k_calm =
#      the first ADMM iteration at which the ensemble shows ANY sensitivity: a count differs between two members, or the
#      violation's relative range exceeds 1e-9.  Before k_calm the GPU must reproduce the strict oracle's counts EXACTLY and
#      its violation to 1e-9: the kernel's whole discrete path, decision by decision, wherever the algorithm allows checking it.
#  (b) PER-PROBLEM ENSEMBLE BOUND.  From k_calm on the reference algorithm amplifies one ulp to 1e-4 .. 1e-2 within an ADMM
#      iteration or two (the onset is sharp: tools/chaos_ensemble.py prints it).  There the GPU's violation after every ADMM
#      iteration must lie within K_SPREAD x the ensemble's range at THAT iteration, and its final X, F within K_SPREAD x the
#      largest pairwise distance among the members on THAT problem (floors 1e-9 / north_star's 1e-5).  No problem borrows another
#      problem's spread.
N_MEMBERS = 16
ENSEMBLE_SEED = 20250204
CALM_HIST = 1e-9


def ulp_perturbed_x_init(b, global_index, member):
    """x_init of every problem moved by one ulp per component, direction drawn from (ENSEMBLE_SEED, global problem index, member)"""
    xi = np.array(b.x_init, dtype=np.float64)
    for i in range(b.B):
        up = np.random.default_rng([ENSEMBLE_SEED, int(global_index[i]), int(member)]).integers(0, 2, size=xi.shape[1]) > 0
        xi[i] = np.nextafter(xi[i], np.where(up, np.inf, -np.inf))
    return xi


def chaos_ensemble(b, global_index, iters, oracle, members=N_MEMBERS, extra=(), **kw):
    """The CPU ensemble of batch b (problems global_index of their config).  Returns the strict result `ref` (with hist / trace)
    and per problem: k_calm, hist_spread [iters] (relative range of the violation per ADMM iteration), spread (largest
    pairwise rel-L2 distance in X and F), count_range [iters] (largest range of a running count).  extra: more member results
    (the numpy twin's, from tools/chaos_ensemble.py)."""
    ref = oracle.solve_batch(b, num_iters=iters, trace=True, **kw)
    runs = [ref, oracle.solve_batch(b, num_iters=iters, trace=True, fast=True, **kw)]
    for k in range(members):
        xi = ulp_perturbed_x_init(b, global_index, k)
        runs.append(oracle.solve_batch(b, num_iters=iters, trace=True, x_init=xi, **kw))
        runs.append(oracle.solve_batch(b, num_iters=iters, trace=True, x_init=xi, fast=True, **kw))
    runs += list(extra)
    return ref, ensemble_summary(runs)


def ensemble_summary(runs):
    ref = runs[0]
    hist = np.stack([r["hist"] for r in runs])             # [M][n][iters], NaN where an iteration did not run
    trace = np.stack([r["trace"] for r in runs])           # [M][n][iters][4], -1 where none ran
    n, iters = hist.shape[1], hist.shape[2]
    ran = ~np.isnan(hist)
    same_ran = np.all(ran == ran[0], axis=0)               # every member ran (or did not run) this iteration
    import warnings
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # iterations nobody ran: all-NaN slices, range 0 below
        hs = (np.nanmax(hist, axis=0) - np.nanmin(hist, axis=0)) / np.abs(ref["hist"])
    hs = np.where(np.isnan(hs), 0.0, hs)
    cr = (trace.max(axis=0) - trace.min(axis=0)).max(axis=2)          # [n][iters]
    sens = (~same_ran) | (cr != 0) | (hs > CALM_HIST)
    k_calm = np.where(sens.any(axis=1), sens.argmax(axis=1), iters)
    spread = np.zeros(n)
    X = np.stack([r["X"] for r in runs])
    F = np.stack([r["F"] for r in runs])
    for a in range(len(runs)):
        for c in range(a + 1, len(runs)):
            spread = np.maximum(spread, np.maximum(rel_l2(X[a], X[c]), rel_l2(F[a], F[c])))
    return dict(k_calm=k_calm.astype(np.int64), hist_spread=hs, spread=spread, count_range=cr.astype(np.int64))


def prefix_parity(got, ref, ens):
    """GPU result `got` (with hist / trace: keep_hist=True) against the strict oracle `ref` under the ensemble summary `ens`.
    Returns (ok [n] bool, report): ok[i] = problem i meets (a) and (b) above; report names what failed, for the assertion text."""
    n, iters = ref["hist"].shape
    e = np.maximum(rel_l2(got["X"], ref["X"]), rel_l2(got["F"], ref["F"]))
    bound = np.maximum(TOL_FP64, K_SPREAD * ens["spread"])
    ok = e <= bound
    why = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        hd = np.abs(got["hist"] - ref["hist"]) / np.abs(ref["hist"])
    for i in range(n):
        kc = int(ens["k_calm"][i])
        msgs = []
        if not np.array_equal(got["trace"][i, :kc], ref["trace"][i, :kc]):
            msgs.append("counts differ inside the calm prefix (k_calm %d): gpu %s ref %s" % (kc, got["trace"][i, :kc].tolist(), ref["trace"][i, :kc].tolist()))
        if not np.array_equal(np.isnan(got["hist"][i]), np.isnan(ref["hist"][i])) and kc >= iters:
            msgs.append("ADMM iterations run differ on a calm problem")
        if np.any(hd[i, :kc] > CALM_HIST):
            msgs.append("violation differs inside the calm prefix: %s" % hd[i, :kc])
        both = ~np.isnan(got["hist"][i, kc:]) & ~np.isnan(ref["hist"][i, kc:])
        lim = np.maximum(CALM_HIST, K_SPREAD * ens["hist_spread"][i, kc:])
        if np.any(hd[i, kc:][both] > lim[both]):
            msgs.append("violation outside %g x the ensemble's range after k_calm %d: %s vs %s" % (K_SPREAD, kc, hd[i, kc:], lim))
        if e[i] > bound[i]:
            msgs.append("final distance %.2e > bound %.2e (own ensemble spread %.2e)" % (e[i], bound[i], ens["spread"][i]))
        if msgs:
            ok[i] = False
            why[i] = msgs
    return ok, dict(err=e, bound=bound, why=why)
