"""Per-knot block-diagonal Q in set_cost_x / set_cost_f on the GPU (run with -m gpu): the block-cost kernel against the CPU
restatement with a general Q (tests/blockq_np.py), against the diagonal kernel where the blocks hold a diagonal, and the dispatch.

The blocks are problems.block_costs': every 3-vector's weights rotated by a seeded yaw in [-1, 1] rad, and for F the Laplacian term
with 0.25 of the knot's mean weight.  For that construction the restatement's own two accumulation orders (Q held sparse / dense)
agree on every count at every horizon used here, cold and warm, and on the iterates to 7e-15 -- except the four-feet H = 63 case,
where the horizon amplifies rounding to ~1e-5 inside the first ADMM iteration (as tests/test_biconvex_gpu.py's
test_horizons_and_ragged_batches notes): that horizon is held to 10 x the spread of the two CPU runs, like there."""
import numpy as np
import pytest
import scipy.sparse as sp

from bunmpc_amd import batch as bb
from bunmpc_amd import problems
from tests import blockq_np
from tests.util import LF, LX, MAPPINGS, TOL_FP64, assert_matches_twin, knobs, launch_record, rel_l2  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu
BQ = "biconvex_admm_bq_kernel"
ALL = ("X", "F", "P", "L_x", "L_f", "stats", "hist", "trace", "dyn_viol")


def _case(oracle, config, B, H=None, seed=7):
    b = problems.make_batch(config, B, H=H) if H else problems.make_batch(config, B)
    pre = oracle.solve_batch(b, num_iters=0)
    blk = problems.block_costs(pre["Qx"], pre["qx"], pre["Qf"], b.E, np.random.default_rng(seed).uniform(-1, 1, B), lam=0.25)
    raw = dict(qx=blk["qx"], lbx=pre["lbx"], ubx=pre["ubx"], Qx_blk=blk["Qx_blk"], Qf_blk=blk["Qf_blk"])
    return b, pre, blk, raw


@pytest.mark.parametrize("mode", ["cold", "warm"])
@pytest.mark.parametrize("H,lanes", MAPPINGS)
@pytest.mark.parametrize("config", ["solo12_trot", "biped_walk"])
def test_block_kernel_matches_the_restatement(oracle, hiplib, knobs, config, H, lanes, mode):
    """every lanes-per-problem mapping, both foot counts, cold and with the warm start and step constants that force retries in both
    FISTA loops: counts and step constants equal, iterates to 1e-5 (H = 63: one ADMM iteration, 10 x the CPU runs' spread)"""
    knobs("bmpc_set_three_per_wave", 1 if lanes == 21 else 0)
    iters = 1 if H == 63 else 3
    b, pre, blk, raw = _case(oracle, config, 6, H)
    kw = dict(warm=b.warm_start(), L_x=LX, L_f=LF) if mode == "warm" else {}
    got = bb.solve_host(b, num_iters=iters, raw=raw, **kw)
    assert launch_record(hiplib) == (BQ, lanes, 1)
    kwi = [dict(warm=kw["warm"], L_x=LX[i], L_f=LF[i]) if mode == "warm" else {} for i in range(b.B)]
    twins = [blockq_np.solve_problem(b, i, pre, blk, iters, **kwi[i]) for i in range(b.B)]
    dense = None
    if H == 63:      # the two accumulation orders of the restatement itself
        dense = [blockq_np.solve_problem(b, i, pre, blk, iters, sparse=False, **kwi[i]) for i in range(b.B)]
    retries = assert_matches_twin(got, twins, spread_of=dense, disagree=dense, tag="%s %d %d %s" % (config, H, lanes, mode))
    assert retries > 0 or mode == "cold"


@pytest.mark.parametrize("config", ["solo12_trot", "biped_walk"])
def test_diagonal_weights_as_blocks_match_the_diagonal_kernel(oracle, hiplib, knobs, config):
    knobs("bmpc_set_latency_mapping_max_batch", 0)
    b = problems.make_batch(config, 6)
    pre = oracle.solve_batch(b, num_iters=0)
    raw = {k: pre[k] for k in ("Qx", "qx", "lbx", "ubx", "Qf")}
    flat = problems.block_costs(pre["Qx"], pre["qx"], pre["Qf"], b.E, yaw=0.0, lam=0.0)
    kw = dict(num_iters=3, warm=b.warm_start(), L_x=LX, L_f=LF)
    ref = bb.solve_host(b, raw=raw, **kw)
    assert launch_record(hiplib)[0] == "biconvex_admm_kernel"
    assert ref["stats"][:, 3].sum() > 0 and ref["stats"][:, 4].sum() > 0
    for sides in (("Qx_blk", "Qf_blk"), ("Qx_blk",), ("Qf_blk",)):      # a side without blocks: its diagonal, spread by the kernel
        got = bb.solve_host(b, raw=dict(raw, **{k: flat[k] for k in sides}), **kw)
        assert launch_record(hiplib)[0] == BQ
        assert np.array_equal(got["stats"], ref["stats"]), sides
        for k in "XFP":
            print(config, sides, k, rel_l2(got[k], ref[k]).max())
            assert np.all(rel_l2(got[k], ref[k]) < TOL_FP64), (sides, k)


def test_shared_blocks_equal_tiled_blocks(oracle, hiplib):
    b, pre, blk, raw = _case(oracle, "solo12_trot", 7)
    shared = dict(raw, Qx_blk=blk["Qx_blk"][2:3], Qf_blk=blk["Qf_blk"][2:3])
    tiled = dict(raw, Qx_blk=np.repeat(blk["Qx_blk"][2:3], 7, axis=0), Qf_blk=np.repeat(blk["Qf_blk"][2:3], 7, axis=0))
    kw = dict(num_iters=3, warm=b.warm_start(), L_x=np.resize(LX, 7), L_f=np.resize(LF, 7), keep_hist=True)
    a, t = bb.solve_host(b, raw=shared, **kw), bb.solve_host(b, raw=tiled, **kw)
    assert launch_record(hiplib)[0] == BQ
    for k in ALL:
        assert np.array_equal(a[k], t[k], equal_nan=True), k
    assert a["stats"][:, 3:5].sum() > 0


@pytest.mark.parametrize("knob,values,iters", [("bmpc_set_certified_steps", (0, 1), 3), ("bmpc_set_exact_step_decisions", (0, 1), 3),
                                               ("bmpc_set_work_stealing", (0, 1), 30), ("bmpc_set_two_waves_per_simd", (0, 1), 3)])
def test_switches_do_not_change_block_results(oracle, hiplib, knobs, knob, values, iters):
    b, pre, blk, raw = _case(oracle, "solo12_trot", 12)
    out = []
    for v in values:
        knobs(knob, v)
        out.append(bb.solve_host(b, num_iters=iters, raw=raw, warm=b.warm_start(), L_x=np.resize(LX, 12), L_f=np.resize(LF, 12), keep_hist=True))
        assert launch_record(hiplib)[0] == BQ and launch_record(hiplib)[2] == 1
    for k in ("X", "F", "P", "stats", "hist", "trace"):
        assert np.array_equal(out[0][k], out[1][k], equal_nan=True), k


def test_dispatch_of_block_batches(oracle, hiplib):
    """B = 1 and B = 4096: the block kernel with blocks, what they take today without"""
    for B, today in ((1, "biconvex_latency_kernel"), (4096, "biconvex_admm_kernel")):
        b = problems.make_batch("solo12_trot", B)
        pre = oracle.solve_batch(b, num_iters=0)
        raw = {k: pre[k] for k in ("Qx", "qx", "lbx", "ubx", "Qf")}
        blk = problems.block_costs(pre["Qx"][:1], pre["qx"][:1], pre["Qf"][:1], b.E, yaw=0.4)
        for iters in (1, 30):
            bb.solve_host(b, num_iters=iters, raw=dict(raw, Qx_blk=blk["Qx_blk"], Qf_blk=blk["Qf_blk"]))
            assert launch_record(hiplib)[0] == BQ, (B, iters)
        bb.solve_host(b, num_iters=1, raw=raw)
        assert launch_record(hiplib)[0] == today, B
    assert hiplib.bmpc_biconvex_block_kernel_scratch_bytes(4) >= 0 and hiplib.bmpc_biconvex_block_kernel_scratch_bytes(2) >= 0


def test_device_batch_carries_blocks(oracle, hiplib):
    b, pre, blk, raw = _case(oracle, "biped_walk", 5)
    host = bb.solve_host(b, num_iters=3, raw=raw)
    dev = bb.DeviceBatch(b, device="cuda:0", num_iters=3, raw=raw)
    dev.solve()
    got = dev.results()
    assert launch_record(hiplib)[0] == BQ
    for k in ("X", "F", "P", "L_x", "L_f", "stats"):
        assert np.array_equal(got[k], host[k]), k


def test_block_calls_without_blocks_are_the_plain_calls(oracle, hiplib):
    """both pointers NULL (or no struct at all): the existing call, kernel and bits"""
    import ctypes as C

    import torch

    from bunmpc_amd import _lib
    b = problems.make_batch("solo12_trot", 9)
    dev = bb.DeviceBatch(b, device="cuda:0", num_iters=3)
    dev.solve()
    want, kernel = dev.results(), launch_record(hiplib)
    stream = C.c_void_p(torch.cuda.current_stream(dev.device).cuda_stream)
    for c in (C.byref(_lib.BlockCost()), None):
        dev.X.zero_()
        _lib.check(hiplib.bmpc_biconvex_solve_batch_blocks_device(C.byref(dev.desc), c, stream))
        got = dev.results()
        assert launch_record(hiplib) == kernel and kernel[0] != BQ
        for k in ("X", "F", "P", "L_x", "L_f", "stats"):
            assert np.array_equal(got[k], want[k]), k


def _drive(mp, b, i, pre, Qx, qx, Qf, iters):
    for t in range(b.H):
        mp.set_contact_plan(b.cnt_plan[i, t], b.dt[i, t])
    mp.set_bounds_x(pre["lbx"][i], pre["ubx"][i])
    if Qx is not None:
        mp.set_cost_x(Qx, qx)
    if Qf is not None:
        mp.set_cost_f(Qf, np.zeros(mp.nf))
    X0, F0, P0 = b.warm_start()
    mp.set_warm_start_vars(X0[i], F0[i], P0[i])
    mp.set_step_constants(LX[i], LF[i])
    mp.optimize(b.x_init[i], iters)
    return dict(X=mp.return_opt_x(), F=mp.return_opt_f(), P=mp.return_opt_p(), stats=mp.last_stats(), L=mp.step_constants())


def test_dropin_takes_sparse_block_costs(oracle, hiplib):
    """BiconvexMP(m, 20, 4) with scipy.sparse block Q_x and Q_f against the restatement; then a diagonal on the same handle: a fresh
    diagonal handle's result, bit for bit"""
    from bunmpc_amd.biconvex_mpc_cpp import BiconvexMP
    b, pre, blk, raw = _case(oracle, "solo12_trot", 6, 20)
    assert b.H == 20 and b.E == 4
    for i in (1, 3):
        Qx, Qf = sp.block_diag(list(blk["Qx_blk"][i]), format="csr"), sp.block_diag(list(blk["Qf_blk"][i]), format="csc")
        mp = BiconvexMP(b.m, 20, 4)
        mp.set_rho(b.rho)
        got = _drive(mp, b, i, pre, Qx, blk["qx"][i], Qf, 3)
        assert launch_record(hiplib)[0] == BQ
        r = blockq_np.solve_problem(b, i, pre, blk, 3, warm=b.warm_start(), L_x=LX[i], L_f=LF[i])
        assert np.array_equal(got["stats"], r["stats"]) and got["L"] == (r["L_x"], r["L_f"])
        assert r["stats"][3] + r["stats"][4] > 0
        for k in "XFP":
            assert rel_l2(got[k], r[k]) < TOL_FP64, (i, k)
        fresh = BiconvexMP(b.m, 20, 4)
        fresh.set_rho(b.rho)
        want = _drive(fresh, b, i, pre, pre["Qx"][i], pre["qx"][i], sp.diags(pre["Qf"][i]), 3)
        assert launch_record(hiplib)[0] != BQ
        # the same handle: X back to a diagonal while F keeps its blocks is still the block kernel; both diagonal: the diagonal path
        _drive(mp, b, i, pre, np.diag(pre["Qx"][i]), pre["qx"][i], None, 3)
        assert launch_record(hiplib)[0] == BQ
        again = _drive(mp, b, i, pre, pre["Qx"][i], pre["qx"][i], pre["Qf"][i], 3)
        assert launch_record(hiplib)[0] != BQ
        for k in ("X", "F", "P", "stats"):
            assert np.array_equal(again[k], want[k]), (i, k)
        assert again["L"] == want["L"]
    with pytest.raises(ValueError, match=r"\(8, 9\)"):
        Q = problems.block_diag_matrix(blk["Qx_blk"][0])
        Q[8, 9] = Q[9, 8] = 1.0
        BiconvexMP(b.m, 20, 4).set_cost_x(sp.csr_matrix(Q), blk["qx"][0])
