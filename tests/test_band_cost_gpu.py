"""Costs between neighbouring knots (force-rate, momentum-rate: "band" Q) on the GPU (run with -m gpu): the band-cost kernel against
the CPU restatement with a general Q (tests/blockq_np.py), against the diagonal kernel where the coupling weights are zero, the
isolation of a wave's problems from a diverging wave-mate, and the dispatch.

The costs are problems.rate_costs': a force-rate term with lam_f x the knot's force weights and a rate term on velocity and angular
momentum with lam_x x the knot's state weights.  With (lam_f, lam_x) = (0.5, 0.5) the restatement's two accumulation orders (Q held
sparse / dense) agree on every count and step constant at every horizon used here, cold and warm, and on the iterates to 7e-15 --
except the four-feet H = 63 case, where the horizon amplifies rounding inside the first ADMM iteration (problem 3: 2e-5): that horizon
is held to max(1e-5, K_SPREAD x the spread of the two CPU runs), as in tests/test_block_cost_gpu.py.  With (4.0, 2.0) the two-feet
cold starts backtrack in the force loop; there one problem of one case (biped_walk, H = 3, warm, problem 5) bifurcates between the two CPU
orders themselves: the strong-weights test leaves out a problem whose two CPU orders disagree on the counts, at most one per case of
six, and prints which."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from bunmpc_amd import batch as bb
from bunmpc_amd import problems
from tests import bandq
from tests.test_block_cost_gpu import _drive
from tests.util import LF, LX, MAPPINGS, TOL_FP64, assert_matches_twin, knobs, launch_record, rel_l2  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu
KQ = "biconvex_admm_kq_kernel"
ALL = ("X", "F", "P", "L_x", "L_f", "stats", "hist", "trace", "dyn_viol")


def _against_restatement(oracle, hiplib, knobs, config, H, lanes, mode, lam, sides="xf", may_skip=0):
    """one case of six problems: counts and step constants equal, iterates within the bound; returns the restatement's retries.
    may_skip: how many problems whose two CPU orders disagree on the counts may be left out (printed)"""
    knobs("bmpc_set_three_per_wave", 1 if lanes == 21 else 0)
    iters = 1 if H == 63 else 3
    b, pre, rc, raw = bandq.case(oracle, config, 6, H, lam=lam, sides=sides)
    kw = dict(warm=b.warm_start(), L_x=LX, L_f=LF) if mode == "warm" else {}
    got = bb.solve_host(b, num_iters=iters, raw=raw, **kw)
    assert launch_record(hiplib) == (KQ, lanes, 1)
    kwi = [dict(warm=kw["warm"], L_x=LX[i], L_f=LF[i]) if mode == "warm" else {} for i in range(b.B)]
    twins = [bandq.restatement(b, i, raw, iters, **kwi[i]) for i in range(b.B)]
    dense = None
    if H == 63 or may_skip:      # the two accumulation orders of the restatement itself
        dense = [bandq.restatement(b, i, raw, iters, sparse=False, **kwi[i]) for i in range(b.B)]
    return assert_matches_twin(got, twins, spread_of=dense if H == 63 else None, may_skip=may_skip, disagree=dense,
                               tag="%s %d %d %s %s %s" % (config, H, lanes, mode, lam, sides))


@pytest.mark.parametrize("mode", ["cold", "warm"])
@pytest.mark.parametrize("H,lanes", MAPPINGS)
@pytest.mark.parametrize("config", ["solo12_trot", "biped_walk"])
def test_band_kernel_matches_the_restatement(oracle, hiplib, knobs, config, H, lanes, mode):
    """every lanes-per-problem mapping, both foot counts, cold and with the warm start and step constants that force retries in both
    FISTA loops, coupling on both sides, (lam_f, lam_x) = (0.5, 0.5): nothing left out"""
    retries = _against_restatement(oracle, hiplib, knobs, config, H, lanes, mode, bandq.MAIN)
    assert retries > 0 or mode == "cold"


@pytest.mark.parametrize("sides", ["x", "f"])
@pytest.mark.parametrize("H,lanes", [(15, 16), (20, 21), (20, 32)])
@pytest.mark.parametrize("config", ["solo12_trot", "biped_walk"])
def test_coupling_on_one_side_only(oracle, hiplib, knobs, config, H, lanes, sides):
    assert _against_restatement(oracle, hiplib, knobs, config, H, lanes, "warm", bandq.MAIN, sides=sides) > 0


@pytest.mark.parametrize("mode", ["cold", "warm"])
@pytest.mark.parametrize("H,lanes", MAPPINGS)
@pytest.mark.parametrize("config", ["solo12_trot", "biped_walk"])
def test_strong_coupling_runs_the_retry_path(oracle, hiplib, knobs, config, H, lanes, mode):
    """(lam_f, lam_x) = (4.0, 2.0): the two-feet cold starts backtrack in the force loop (the restatement's L_f 506.25 -> 759.375, at
    H = 63 -> 1139.0625) with the coupling in it; the four-feet cold starts take no retry below H = 63.  A problem whose two CPU orders
    disagree on the counts may be left out, at most one per case"""
    retries = _against_restatement(oracle, hiplib, knobs, config, H, lanes, mode, bandq.STRONG, may_skip=1)
    assert retries > 0 or (mode == "cold" and config == "solo12_trot" and H < 63)


@pytest.mark.parametrize("config", ["solo12_trot", "biped_walk"])
def test_zero_coupling_matches_the_diagonal_kernel(oracle, hiplib, knobs, config):
    """arrays present, all zeros, one side or both: the diagonal raw kernel's discrete path and its iterates to 1e-5 (whether the bits
    are equal too is printed); the warm batches with retries in both loops"""
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    b = problems.make_batch(config, 6)
    pre = oracle.solve_batch(b, num_iters=0)
    raw = {k: pre[k] for k in ("Qx", "qx", "lbx", "ubx", "Qf")}
    zero = dict(Qx_off=np.zeros((6, b.H, 9)), Qf_off=np.zeros((6, b.H - 1, 3 * b.E)))
    kw = dict(num_iters=3, warm=b.warm_start(), L_x=LX, L_f=LF)
    ref = bb.solve_host(b, raw=raw, **kw)
    assert launch_record(hiplib)[0] == "biconvex_admm_kernel"
    assert ref["stats"][:, 3].sum() > 0 and ref["stats"][:, 4].sum() > 0
    for sides in (("Qx_off", "Qf_off"), ("Qx_off",), ("Qf_off",)):
        got = bb.solve_host(b, raw=dict(raw, **{k: zero[k] for k in sides}), **kw)
        assert launch_record(hiplib)[0] == KQ
        assert np.array_equal(got["stats"], ref["stats"]), sides
        assert np.array_equal(got["L_x"], ref["L_x"]) and np.array_equal(got["L_f"], ref["L_f"]), sides
        for k in "XFP":
            print("ZERO", config, sides, k, "max rel_l2", rel_l2(got[k], ref[k]).max(), "bits equal:", np.array_equal(got[k], ref[k]))
            assert np.all(rel_l2(got[k], ref[k]) < TOL_FP64), (sides, k)


def test_band_calls_without_coupling_are_the_plain_calls(hiplib):
    """both pointers NULL (or no struct at all): the existing call, kernel and bits"""
    import torch

    from bunmpc_amd import _lib
    b = problems.make_batch("solo12_trot", 9)
    dev = bb.DeviceBatch(b, device="cuda:0", num_iters=3)
    dev.solve()
    want, kernel = dev.results(), launch_record(hiplib)
    stream = C.c_void_p(torch.cuda.current_stream(dev.device).cuda_stream)
    for c in (C.byref(_lib.BandCost()), None):
        dev.X.zero_()
        _lib.check(hiplib.bmpc_biconvex_solve_batch_band_device(C.byref(dev.desc), c, stream))
        got = dev.results()
        assert launch_record(hiplib) == kernel and kernel[0] != KQ
        for k in ("X", "F", "P", "L_x", "L_f", "stats"):
            assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("config", ["solo12_trot", "biped_walk"])
def test_a_diverging_problem_leaves_its_wave_mates_alone(oracle, hiplib, knobs, config):
    """21-lane segments, three problems per wave: the middle problem of each wave's three overflows (x_init and qx at 1e200, coupling on
    both sides: its NaNs reach its neighbours' lanes through the wave shifts) -- status 2 for it, and its wave-mates bit for bit what
    they are in the clean batch"""
    knobs("bmpc_set_three_per_wave", 1)
    b, pre, rc, raw = bandq.case(oracle, config, 6, 20)
    bad_b, _, _, bad_raw = bandq.case(oracle, config, 6, 20)
    bad_raw["qx"] = np.array(bad_raw["qx"])
    for i in (1, 4):
        bad_b.x_init[i, 2] = 1e200
        bad_raw["qx"][i] = 1e200
    clean = bb.solve_host(b, num_iters=4, raw=raw)
    assert launch_record(hiplib) == (KQ, 21, 1)
    got = bb.solve_host(bad_b, num_iters=4, raw=bad_raw)
    assert launch_record(hiplib) == (KQ, 21, 1)
    for i in (1, 4):
        assert got["stats"][i, 5] == 2, got["stats"][i]
        assert not np.isfinite(got["X"][i]).all()
    for i in (0, 2, 3, 5):
        assert got["stats"][i, 5] == 0
        assert np.array_equal(got["stats"][i], clean["stats"][i]), i
        for k in "XFP":
            assert np.array_equal(got[k][i], clean[k][i]), (i, k)


def test_shared_coupling_equals_tiled_coupling(oracle, hiplib):
    b, pre, rc, raw = bandq.case(oracle, "solo12_trot", 7)
    shared = dict(raw, Qx_off=rc["Qx_off"][2:3], Qf_off=rc["Qf_off"][2:3])
    tiled = dict(raw, Qx_off=np.repeat(rc["Qx_off"][2:3], 7, axis=0), Qf_off=np.repeat(rc["Qf_off"][2:3], 7, axis=0))
    kw = dict(num_iters=3, warm=b.warm_start(), L_x=np.resize(LX, 7), L_f=np.resize(LF, 7), keep_hist=True)
    a, t = bb.solve_host(b, raw=shared, **kw), bb.solve_host(b, raw=tiled, **kw)
    assert launch_record(hiplib)[0] == KQ
    for k in ALL:
        assert np.array_equal(a[k], t[k], equal_nan=True), k
    assert a["stats"][:, 3:5].sum() > 0


@pytest.mark.parametrize("knob,values,iters", [("bmpc_set_certified_steps", (0, 1), 3), ("bmpc_set_exact_step_decisions", (0, 1), 3),
                                               ("bmpc_set_work_stealing", (0, 1), 30), ("bmpc_set_two_waves_per_simd", (0, 1), 3)])
def test_switches_do_not_change_band_results(oracle, hiplib, knobs, knob, values, iters):
    b, pre, rc, raw = bandq.case(oracle, "solo12_trot", 12)
    out = []
    for v in values:
        knobs(knob, v)
        out.append(bb.solve_host(b, num_iters=iters, raw=raw, warm=b.warm_start(), L_x=np.resize(LX, 12), L_f=np.resize(LF, 12), keep_hist=True))
        assert launch_record(hiplib)[0] == KQ and launch_record(hiplib)[2] == 1
    for k in ("X", "F", "P", "stats", "hist", "trace"):
        assert np.array_equal(out[0][k], out[1][k], equal_nan=True), k


def test_dispatch_of_band_batches(oracle, hiplib):
    """B = 1 and B = 4096, num_iters 1 and 30: the band kernel with coupling (a problem's result does not depend on the batch around
    it), what they take today without"""
    first = {}
    for B, today in ((1, "biconvex_latency_kernel"), (4096, "biconvex_admm_kernel")):
        b = problems.make_batch("solo12_trot", B)
        pre = oracle.solve_batch(b, num_iters=0)
        rc = problems.rate_costs(pre["Qx"], pre["Qf"], b.E, lam_x=0.5, lam_f=0.5)
        raw = dict(Qx=rc["Qx"], qx=pre["qx"], lbx=pre["lbx"], ubx=pre["ubx"], Qf=rc["Qf"], Qx_off=rc["Qx_off"], Qf_off=rc["Qf_off"])
        for iters in (1, 30):
            got = bb.solve_host(b, num_iters=iters, raw=raw)
            assert launch_record(hiplib)[0] == KQ and launch_record(hiplib)[2] == 1, (B, iters)
            if B == 1:
                first[iters] = got
            else:
                for k in ("X", "F", "P", "L_x", "L_f", "stats"):
                    assert np.array_equal(got[k][0], first[iters][k][0]), (iters, k)
        bb.solve_host(b, num_iters=1, raw={k: pre[k] for k in ("Qx", "qx", "lbx", "ubx", "Qf")})
        assert launch_record(hiplib)[0] == today, B
    s4, s2 = hiplib.bmpc_biconvex_band_kernel_scratch_bytes(4), hiplib.bmpc_biconvex_band_kernel_scratch_bytes(2)
    print("SCRATCH bytes per lane: four feet", s4, "two feet", s2)
    assert s4 >= 0 and s2 >= 0


def test_device_batch_carries_coupling(oracle, hiplib):
    b, pre, rc, raw = bandq.case(oracle, "biped_walk", 5)
    host = bb.solve_host(b, num_iters=3, raw=raw)
    dev = bb.DeviceBatch(b, device="cuda:0", num_iters=3, raw=raw)
    dev.solve()
    got = dev.results()
    assert launch_record(hiplib)[0] == KQ
    for k in ("X", "F", "P", "L_x", "L_f", "stats"):
        assert np.array_equal(got[k], host[k]), k


@pytest.mark.parametrize("config,E", [("solo12_trot", 4), ("biped_walk", 2)])
def test_dropin_takes_sparse_band_costs(oracle, hiplib, config, E):
    """BiconvexMP(m, 20, E) with scipy.sparse band Q_x and Q_f against the restatement; then a diagonal on the same handle: a fresh
    diagonal handle's result, bit for bit"""
    from bunmpc_amd.biconvex_mpc_cpp import BiconvexMP
    b, pre, rc, raw = bandq.case(oracle, config, 6, 20)
    assert b.H == 20 and b.E == E
    for i in (1, 3):
        Qx, Qf = bandq.matrices(raw, i, E)
        mp = BiconvexMP(b.m, 20, E)
        mp.set_rho(b.rho)
        got = _drive(mp, b, i, pre, sp.csr_matrix(Qx), pre["qx"][i], sp.csc_matrix(Qf), 3)
        assert launch_record(hiplib)[0] == KQ
        r = bandq.restatement(b, i, raw, 3, warm=b.warm_start(), L_x=LX[i], L_f=LF[i])
        print(config, i, got["stats"].tolist(), r["stats"].tolist(), {k: rel_l2(got[k], r[k]) for k in "XFP"})
        assert np.array_equal(got["stats"], r["stats"]) and got["L"] == (r["L_x"], r["L_f"])
        assert r["stats"][3] + r["stats"][4] > 0
        for k in "XFP":
            assert rel_l2(got[k], r[k]) < TOL_FP64, (i, k)
        fresh = BiconvexMP(b.m, 20, E)
        fresh.set_rho(b.rho)
        want = _drive(fresh, b, i, pre, pre["Qx"][i], pre["qx"][i], sp.diags(pre["Qf"][i]), 3)
        assert launch_record(hiplib)[0] != KQ
        # the same handle: X back to a diagonal while F keeps its coupling is still the band kernel; both diagonal: the diagonal path
        _drive(mp, b, i, pre, np.diag(pre["Qx"][i]), pre["qx"][i], None, 3)
        assert launch_record(hiplib)[0] == KQ
        again = _drive(mp, b, i, pre, pre["Qx"][i], pre["qx"][i], pre["Qf"][i], 3)
        assert launch_record(hiplib)[0] != KQ
        for k in ("X", "F", "P", "stats"):
            assert np.array_equal(again[k], want[k]), (i, k)
        assert again["L"] == want["L"]
