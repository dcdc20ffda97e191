"""The CPU twin of the fp32 centroidal kernels (tests/f32_np.py) is fit to judge them: on every problem of every case and regime all ten
members of the twin's ensemble and the strict fp64 C oracle take the same discrete path with every decision clear of its threshold; run in
fp64 the twin is the reference's algebra; and twins with one fault each fall outside what tests/test_f32_gpu.py accepts."""
import numpy as np
import pytest

from tests import cone_np, f32_np
from tests.util import problem_args, rel_l2
from oracle import oracle_np

CASE_IDS = [f32_np.case_id(c) for c in f32_np.CASES]
CARRIED = (32, 20, 5, "solo12_trot")        # the case tests/test_f32_gpu.py runs with carried step constants (regime k)


def test_cases_reach_all_six_instantiations():
    """LPP in {16, 32, 64} x E in {2, 4}; B ragged against the problems per wave"""
    assert {(c[0], f32_np.batch(c)[0].E) for c in f32_np.CASES} == {(l, e) for l in (16, 32, 64) for e in (2, 4)}
    for lanes, H, B, _ in f32_np.CASES:
        assert H + 1 <= lanes and (lanes == 16 or H + 1 > lanes // 2) and (lanes == 64 or B % (64 // lanes) != 0)


@pytest.mark.parametrize("regime", f32_np.REGIMES + ("k",))
@pytest.mark.parametrize("case", f32_np.CASES, ids=CASE_IDS)
def test_twin_is_fit_to_judge(oracle, case, regime):
    """Every member of every problem's ensemble agrees with the strict fp64 oracle on every entry of trace (and on the counts and step
    constants the solve returns), and takes every decision at least f32_np.MARGIN = 1e-4 relative from its threshold: 50 x the bound
    n 2^-24 on a per-lane fp32 sum of n <= 32 non-negative terms.  A condition, not a measurement: a problem that misses it gets another
    seed or tol in tests/f32_np.py (SEEDS, OVERRIDES), none is left out."""
    if regime == "k" and case != CARRIED:
        return
    ens, ref = f32_np.members(case, regime), f32_np.oracle_solve(oracle, case, regime)
    margin = np.min([r["margin"] for r in ens], axis=0)
    print(f32_np.case_id(case), regime, "stats", ref["stats"].tolist(), "smallest margin (force retry, force exit, motion retry, motion exit, ADMM exit)", margin.min(axis=0))
    if regime in "bck":
        assert np.any(ref["stats"][:, 3] > 0), "every case backtracks in the force loop"
    if regime == "c":
        assert np.all(ref["trace"][:, 0, :2].min(axis=1) < f32_np.settings(case, regime)["maxit"]), "the FISTA exit decides"
    for r in ens:
        assert np.array_equal(r["trace"], ref["trace"])
        assert np.array_equal(r["stats"], ref["stats"])
        assert np.array_equal(r["L_x"], ref["L_x"]) and np.array_equal(r["L_f"], ref["L_f"])
        assert np.all(r["margin"] >= f32_np.MARGIN), r["margin"].min(axis=0)


@pytest.mark.parametrize("case", f32_np.R_CASES, ids=[f32_np.case_id(c) for c in f32_np.R_CASES])
def test_retry_decisions_at_the_reference_tolerances(oracle, case):
    """Regime r (tol = 1e-5, maxit = 150, ten ADMM iterations): the exits of fp32 runs do not agree there, the retry decisions do -- every
    member of every problem's ensemble returns the oracle's retry counts, ADMM count, status and step constants, and takes every retry
    decision at least MARGIN from its threshold (smallest over the cases: 6.5e-2)"""
    ens, ref = f32_np.members(case, "r"), f32_np.oracle_solve(oracle, case, "r")
    print(f32_np.case_id(case), "stats", ref["stats"].tolist(), "smallest retry margin", np.min([r["margin"][:, [0, 2]] for r in ens]))
    for r in ens:
        assert np.array_equal(r["stats"][:, [0, 3, 4, 5]], ref["stats"][:, [0, 3, 4, 5]])
        assert np.array_equal(r["L_x"], ref["L_x"]) and np.array_equal(r["L_f"], ref["L_f"])
        assert np.all(r["margin"][:, [0, 2]] >= f32_np.MARGIN)


@pytest.mark.parametrize("regime", ["a", "b"])
@pytest.mark.parametrize("case", [c for c in f32_np.CASES if c[1] <= 20], ids=[i for c, i in zip(f32_np.CASES, CASE_IDS) if c[1] <= 20])
def test_twin_in_fp64_is_the_reference(case, regime):
    """dtype = float64 instead of float32: oracle_np.biconvex_solve to 1e-12 -- the x_init rows folded into knot 0, the momentum table,
    A d for the image difference and the half gradient are the reference's algebra"""
    b, s = f32_np.batch(case)[0], f32_np.settings(case, regime)
    got = f32_np.run(case, regime, dtype=np.float64)
    raw = cone_np.raw_batch(b)
    for i in range(b.B):
        ref = oracle_np.biconvex_solve(*problem_args(b, i, raw, s["warm"]), L_x=s["L_x"][i], L_f=s["L_f"][i], rho=b.rho, num_iters=s["num_iters"],
                                       maxit=s["maxit"], tol=s["tol"], exit_tol=s["exit_tol"], mu=b.mu)
        assert np.array_equal(got["stats"][i], ref["stats"]) and np.array_equal(got["trace"][i], ref["trace"])
        assert got["L_x"][i] == ref["L_x"] and got["L_f"][i] == ref["L_f"]
        err = {k: rel_l2(got[k][i], ref[k]) for k in "XFP"}
        assert max(err.values()) <= 1e-12, (i, err)
        assert np.allclose(got["hist"][i], ref["hist"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("mutant", f32_np.MUTANTS)
def test_mutated_twin_falls_outside_the_bound(oracle, mutant):
    """Teeth: a twin with one fault -- one force weight of one knot scaled by 1 + 1e-4 (weight), A d taken as the difference of the images
    (imagediff), the last knot's lane left out of g2 (droplane) -- run as tests/test_f32_gpu.py runs the kernel must fail its judgement
    (f32_np.judge: the discrete path, then 10 x max(y_i, 2^-23) on the values and on hist) on at least one case.

    weight and droplane do, on the first case tried.  imagediff passes all 39 case-regimes of a, b and c: the difference of the
    images changes nothing but the sum cv of the force step's retry test, by the rounding of the two images (1e-7 of |A y + bPk|, about
    0.5 here, against |A d|, about 0.04 |d|), and where every decision is MARGIN clear of its threshold cv stays on its side in every
    trial -- the unmutated twin's own bits (error / y_i 0.47 .. 1.00, same path).  It shows once steps are a few fp32 ulp of the forces,
    which is regime r: there the mutant's retry test fires on the images' rounding until L_f is +inf (204 retries) on 9 of the 31
    problems of f32_np.R_CASES, against 0 or 1 retries of every member and of the oracle."""
    caught = []
    for regime, case in [(r, c) for c in f32_np.CASES for r in f32_np.REGIMES] + [("r", c) for c in f32_np.R_CASES]:
        ens, ref = f32_np.members(case, regime), f32_np.oracle_solve(oracle, case, regime)
        j = f32_np.judge(f32_np.run(case, regime, mutant=mutant), ens, ref, exact=regime != "r")
        print(mutant, f32_np.case_id(case), regime, "path", j["path"].tolist(), "error / y", np.round(j["ratio"], 2).tolist(), "hist", np.round(j["ratio_hist"], 2).tolist())
        if not j["ok"].all():
            caught.append((f32_np.case_id(case), regime))
            break
    assert caught, "the mutant passes every case"
