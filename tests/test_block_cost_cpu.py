"""Per-knot block-diagonal Q in set_cost_x / set_cost_f, the parts that need no GPU: the CPU restatement with a general Q
(tests/blockq_np.py) pinned to the diagonal one, the structure classification of the Python drop-in, and the argument checks of the
C-ABI's block entry points."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from bunmpc_amd import _lib, problems
from bunmpc_amd.biconvex_mpc_cpp import classify_cost
from tests import blockq_np
from tests.util import TOL_FP64, rel_l2, restatement

BLOCKS = (_lib.BlockCost, lambda H, E: dict(Qx_blk=81 * (H + 1), Qf_blk=9 * E * E * H))


@pytest.mark.parametrize("config", ["solo12_trot", "biped_walk"])
def test_restatement_with_diagonal_blocks_matches_the_diagonal_oracle(oracle, config):
    """the new checker against the existing one: a Q that holds the diagonal alone gives the diagonal restatement's counts and iterates"""
    b = problems.make_batch(config, 2, H=20)
    pre = oracle.solve_batch(b, num_iters=0)
    for i in range(b.B):
        rd = restatement(b, i, pre, 3)
        whole = dict(pre, Qx={i: np.diag(pre["Qx"][i])}, Qf={i: np.diag(pre["Qf"][i])})
        for sparse in (True, False):
            rb = restatement(b, i, whole, 3, problem=blockq_np.PROBLEM[sparse])
            assert np.array_equal(rd["stats"], rb["stats"]), (i, sparse)
            for k in "XFP":
                print(config, i, sparse, k, rel_l2(rb[k], rd[k]))
                assert rel_l2(rb[k], rd[k]) < TOL_FP64, (i, sparse, k)


@pytest.mark.parametrize("E", [2, 4])
def test_block_helper_is_psd_and_reduces_to_the_diagonal(oracle, E):
    b = problems.make_batch("solo12_trot" if E == 4 else "biped_walk", 3, H=5)
    pre = oracle.solve_batch(b, num_iters=0)
    blk = problems.block_costs(pre["Qx"], pre["qx"], pre["Qf"], E, yaw=np.array([0.3, -1.0, 1.0]))
    assert blk["Qx_blk"].shape == (3, 6, 9, 9) and blk["Qf_blk"].shape == (3, 5, 3 * E, 3 * E)
    for a in (blk["Qx_blk"], blk["Qf_blk"]):
        assert np.array_equal(a, a.transpose(0, 1, 3, 2))
        ev = np.linalg.eigvalsh(a)
        assert np.all(ev.min(axis=-1) >= -1e-12 * ev.max(axis=-1))
    assert np.any(blk["Qf_blk"][:, :, 0, 3] != 0)      # the feet are coupled
    flat = problems.block_costs(pre["Qx"], pre["qx"], pre["Qf"], E, yaw=0.0, lam=0.0)
    assert np.array_equal(np.diagonal(flat["Qx_blk"], axis1=2, axis2=3).reshape(3, -1), pre["Qx"])
    assert np.array_equal(np.diagonal(flat["Qf_blk"], axis1=2, axis2=3).reshape(3, -1), pre["Qf"])
    assert np.allclose(flat["qx"], pre["qx"], rtol=1e-15, atol=0)


@pytest.mark.parametrize("E", [2, 4])
@pytest.mark.parametrize("form", ["dense", "csr", "coo"])
def test_structure_classification(E, form):
    H = 4
    rng = np.random.default_rng(5)
    for k, n in ((9, 9 * (H + 1)), (3 * E, 3 * E * H)):
        conv = {"dense": lambda M: M, "csr": sp.csr_matrix, "coo": sp.coo_matrix}[form]
        d = rng.uniform(1, 2, n)
        kind, got = classify_cost(conv(np.diag(d)), n, k, "Q")
        assert kind == "diag" and np.array_equal(got, d)
        if form == "dense":
            kind, got = classify_cost(d, n, k, "Q")
            assert kind == "diag" and np.array_equal(got, d)
        blk = rng.uniform(-1, 1, (n // k, k, k))
        blk = blk + blk.transpose(0, 2, 1)
        Q = problems.block_diag_matrix(blk)
        kind, got = classify_cost(conv(Q), n, k, "Q")
        assert kind == "blocks" and np.array_equal(got, blk)
        wide = Q.copy()
        wide[k - 1, k] = wide[k, k - 1] = 0.5       # one symmetric pair outside its knot's block
        with pytest.raises(ValueError, match=r"\(%d, %d\)" % (k - 1, k)):
            classify_cost(conv(wide), n, k, "Q")
        asym = Q.copy()
        asym[k + 1, k + 2] += 1e-9                  # one asymmetric pair inside a block
        with pytest.raises(ValueError, match=r"\(%d, %d\).*symmetric" % (k + 1, k + 2)):
            classify_cost(conv(asym), n, k, "Q")
        with pytest.raises(ValueError, match="expected"):
            classify_cost(conv(Q[:-1, :-1]), n, k, "Q")


def _descriptor(hiplib, keep, cost, B=1, H=20, E=4):
    """a raw batch descriptor of zeros and ones and a cost struct cost = (class, (H, E) -> {field: doubles}); the arrays go to `keep`"""
    nx, nf = 9 * (H + 1), 3 * E * H
    d = _lib.Batch()
    hiplib.bmpc_batch_defaults(C.byref(d))
    d.B, d.n_col, d.n_eff, d.raw, d.cold_start = B, H, E, 1, 1

    def arr(n, v=0.0):
        a = np.full(n, v)
        keep.append(a)
        return a.ctypes.data
    d.cnt_plan, d.dt, d.x_init = arr(B * H * E * 4), arr(B * H, 0.05), arr(B * 9)
    d.Qx, d.qx, d.lbx, d.ubx, d.Qf = arr(B * nx, 1.0), arr(B * nx), arr(B * nx, -1e9), arr(B * nx, 1e9), arr(B * nf, 1.0)
    d.X, d.F, d.P, d.L_x, d.L_f = arr(B * nx), arr(B * nf), arr(B * nx), arr(B), arr(B)
    c = cost[0]()
    for field, n in cost[1](H, E).items():
        setattr(c, field, arr(n))
    return d, c


def test_block_entry_points_refuse_what_is_not_built(hiplib):
    assert hiplib.bmpc_block_cost_struct_size() == C.sizeof(_lib.BlockCost)
    assert hiplib.bmpc_abi_version() == 2
    keep = []
    for change, word in ((dict(precision=1), "fp64"), (dict(raw=0), "raw"), (dict(n_col=64), "64 knots")):
        H = change.get("n_col", 20)
        d, c = _descriptor(hiplib, keep, BLOCKS, H=H)
        for k, v in change.items():
            setattr(d, k, v)
        for call in (lambda: hiplib.bmpc_biconvex_solve_batch_blocks_host(C.byref(d), C.byref(c)),
                     lambda: hiplib.bmpc_biconvex_solve_batch_blocks_device(C.byref(d), C.byref(c), None)):
            assert call() == _lib.BAD_ARG
            msg = hiplib.bmpc_last_error().decode()
            assert "block costs" in msg and word in msg, msg
    # a stride that is neither shared nor a whole problem's blocks
    d, c = _descriptor(hiplib, keep, BLOCKS)
    c.sQx_blk = 5
    assert hiplib.bmpc_biconvex_solve_batch_blocks_host(C.byref(d), C.byref(c)) == _lib.BAD_ARG
    assert "stride" in hiplib.bmpc_last_error().decode()
    # an asymmetric block on the host entry point and on the handle
    d, c = _descriptor(hiplib, keep, BLOCKS)
    keep[-2][81 * 3 + 1] = 1.0      # Qx_blk, knot 3, (0, 1)
    assert hiplib.bmpc_biconvex_solve_batch_blocks_host(C.byref(d), C.byref(c)) == _lib.BAD_ARG
    assert "not symmetric at (0, 1)" in hiplib.bmpc_last_error().decode()
    h = hiplib.bmpc_biconvex_create(2.5, 20, 4)
    try:
        assert hiplib.bmpc_biconvex_set_cost_x_blocks(h, keep[-2].ctypes.data, np.zeros(189).ctypes.data) == _lib.BAD_ARG
        assert "not symmetric" in hiplib.bmpc_last_error().decode()
        assert hiplib.bmpc_biconvex_set_cost_x_blocks(h, np.zeros(81 * 21).ctypes.data, np.zeros(189).ctypes.data) == _lib.OK
        assert hiplib.bmpc_biconvex_set_cost_f_blocks(h, np.zeros(144 * 20).ctypes.data, np.zeros(240).ctypes.data) == _lib.OK
        assert hiplib.bmpc_biconvex_set_cost_x_blocks(None, None, None) == _lib.BAD_ARG
    finally:
        hiplib.bmpc_biconvex_destroy(h)
    assert hiplib.bmpc_biconvex_block_kernel_scratch_bytes(3) == -1
