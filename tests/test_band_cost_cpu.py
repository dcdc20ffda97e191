"""Costs between neighbouring knots (force-rate, momentum-rate: "band" Q) in set_cost_x / set_cost_f, the parts that need no GPU:
the structure classification of the Python drop-in, the helpers that build the test costs, and the argument checks of the C-ABI's
band entry points and of the handle."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from bunmpc_amd import _lib, problems
from bunmpc_amd.biconvex_mpc_cpp import classify_cost
from tests.test_block_cost_cpu import _descriptor

BAND = (_lib.BandCost, lambda H, E: dict(Qx_off=9 * H, Qf_off=3 * E * (H - 1)))


def _band(rng, n, k, sign=1.0):
    diag = rng.uniform(1, 2, (n // k, k))
    off = sign * rng.uniform(-1, 1, (n // k - 1, k))
    return diag, off


@pytest.mark.parametrize("E", [2, 4])
@pytest.mark.parametrize("form", ["dense", "csr", "coo"])
def test_band_classification(E, form):
    H = 4
    rng = np.random.default_rng(11)
    conv = {"dense": lambda M: M, "csr": sp.csr_matrix, "coo": sp.coo_matrix}[form]
    for k, n in ((9, 9 * (H + 1)), (3 * E, 3 * E * H)):
        diag, off = _band(rng, n, k)
        Q = problems.band_matrix(diag, off)
        assert np.array_equal(Q, Q.T) and np.array_equal(np.diag(Q), diag.reshape(-1))
        kind, got = classify_cost(conv(Q), n, k, "Q")
        assert kind == "band"
        assert got[0].shape == (n // k, k) and got[1].shape == (n // k - 1, k)
        assert np.array_equal(got[0], diag) and np.array_equal(got[1], off)
        # a single coupled pair is a band too; no coupling at all stays a diagonal
        one = np.diag(diag.reshape(-1))
        one[3, 3 + k] = one[3 + k, 3] = -0.25
        kind, got = classify_cost(conv(one), n, k, "Q")
        assert kind == "band" and got[1][0, 3] == -0.25 and np.count_nonzero(got[1]) == 1
        assert classify_cost(conv(np.diag(diag.reshape(-1))), n, k, "Q")[0] == "diag"
        # off the neighbour block's diagonal: the first offending entry in row-major order
        bad = Q.copy()
        bad[k - 1, k] = bad[k, k - 1] = 0.5
        with pytest.raises(ValueError, match=r"\(%d, %d\)" % (k - 1, k)):
            classify_cost(conv(bad), n, k, "Q")
        bad = Q.copy()
        bad[2, 2 * k + 2] = bad[2 * k + 2, 2] = 0.5      # the same component two knots apart
        with pytest.raises(ValueError, match=r"\(2, %d\)" % (2 * k + 2)):
            classify_cost(conv(bad), n, k, "Q")
        bad = Q.copy()
        bad[1, k + 2] = bad[k + 2, 1] = 0.5              # neighbouring knots, different components
        with pytest.raises(ValueError, match=r"\(1, %d\)" % (k + 2)):
            classify_cost(conv(bad), n, k, "Q")
        asym = Q.copy()
        asym[4, 4 + k] += 1e-9
        with pytest.raises(ValueError, match=r"\(4, %d\).*symmetric" % (4 + k)):
            classify_cost(conv(asym), n, k, "Q")
        # coupling next to a per-knot block that is not diagonal
        full = Q.copy()
        full[k + 1, k + 2] = full[k + 2, k + 1] = 0.125
        with pytest.raises(ValueError, match=r"\(%d, %d\).*diagonal per-knot weights" % (k + 1, k + 2)):
            classify_cost(conv(full), n, k, "Q")


@pytest.mark.parametrize("k,n", [(9, 45), (6, 24), (12, 48)])
def test_duplicate_coo_entries_add_up(k, n):
    rng = np.random.default_rng(3)
    diag, off = _band(rng, n, k)
    Q = sp.coo_matrix(problems.band_matrix(diag, off))
    half = sp.coo_matrix((np.concatenate([Q.data * 0.25, Q.data * 0.75]), (np.concatenate([Q.row, Q.row]), np.concatenate([Q.col, Q.col]))), shape=(n, n))
    kind, got = classify_cost(half, n, k, "Q")
    assert kind == "band"
    assert np.allclose(got[0], diag, rtol=1e-15, atol=0) and np.allclose(got[1], off, rtol=1e-15, atol=0)
    assert np.array_equal(got[1], (off * 0.25 + off * 0.75))


@pytest.mark.parametrize("E", [2, 4])
def test_rate_helper_is_psd_and_equals_the_difference_form(oracle, E):
    b = problems.make_batch("solo12_trot" if E == 4 else "biped_walk", 3, H=5)
    pre = oracle.solve_batch(b, num_iters=0)
    lam_x, lam_f = 0.5, 4.0
    rc = problems.rate_costs(pre["Qx"], pre["Qf"], E, lam_x=lam_x, lam_f=lam_f)
    assert rc["Qx"].shape == (3, 54) and rc["Qx_off"].shape == (3, 5, 9) and rc["Qf"].shape == (3, 15 * E) and rc["Qf_off"].shape == (3, 4, 3 * E)
    assert np.all(rc["Qx_off"][:, :, :3] == 0) and np.any(rc["Qx_off"][:, :, 3:] != 0) and np.any(rc["Qf_off"] != 0)
    for i in range(3):
        for name, k, base, lam in (("Qx", 9, pre["Qx"][i], lam_x), ("Qf", 3 * E, pre["Qf"][i], lam_f)):
            Q = problems.band_matrix(rc[name][i], rc[name + "_off"][i])
            n = base.size // k
            assert np.array_equal(Q, Q.T)
            # diag + D'R D built independently: D the first difference over the knots, R the weights of the pairs
            D = np.zeros(((n - 1) * k, n * k))
            for t in range(n - 1):
                D[t * k:(t + 1) * k, t * k:(t + 1) * k] = -np.eye(k)
                D[t * k:(t + 1) * k, (t + 1) * k:(t + 2) * k] = np.eye(k)
            R = lam * base.reshape(n, k)[:-1].copy()
            if name == "Qx":
                R[:, :3] = 0.0
            want = np.diag(base) + D.T @ np.diag(R.reshape(-1)) @ D
            assert np.allclose(Q, want, rtol=1e-14, atol=0)
            ev = np.linalg.eigvalsh(Q)
            assert ev.min() >= -1e-12 * ev.max()
            kind, got = classify_cost(sp.csr_matrix(Q), n * k, k, name)
            assert kind == "band" and np.array_equal(got[0].reshape(-1), rc[name][i]) and np.array_equal(got[1], rc[name + "_off"][i])


def test_band_symbols_are_bound(hiplib):
    for name in ("bmpc_band_cost_struct_size", "bmpc_biconvex_solve_batch_band_device", "bmpc_biconvex_solve_batch_band_host",
                 "bmpc_biconvex_set_cost_x_band", "bmpc_biconvex_set_cost_f_band", "bmpc_biconvex_band_kernel_scratch_bytes"):
        assert name in _lib._SIGS and getattr(hiplib, name)
    assert hiplib.bmpc_band_cost_struct_size() == C.sizeof(_lib.BandCost)
    assert hiplib.bmpc_abi_version() == 2
    assert hiplib.bmpc_biconvex_band_kernel_scratch_bytes(3) == -1


def test_band_entry_points_refuse_what_is_not_built(hiplib):
    keep = []
    for change, word in ((dict(precision=1), "fp64"), (dict(raw=0), "raw"), (dict(n_col=64), "64 knots")):
        H = change.get("n_col", 20)
        d, c = _descriptor(hiplib, keep, BAND, H=H)
        for k, v in change.items():
            setattr(d, k, v)
        for call in (lambda: hiplib.bmpc_biconvex_solve_batch_band_host(C.byref(d), C.byref(c)),
                     lambda: hiplib.bmpc_biconvex_solve_batch_band_device(C.byref(d), C.byref(c), None)):
            assert call() == _lib.BAD_ARG
            msg = hiplib.bmpc_last_error().decode()
            assert "neighbouring knots" in msg and word in msg, msg
    # a stride that is neither shared nor a whole problem's weights
    for field in ("sQx_off", "sQf_off"):
        d, c = _descriptor(hiplib, keep, BAND)
        setattr(c, field, 5)
        assert hiplib.bmpc_biconvex_solve_batch_band_host(C.byref(d), C.byref(c)) == _lib.BAD_ARG
        assert "stride" in hiplib.bmpc_last_error().decode()


def test_handle_refuses_coupling_next_to_blocks(hiplib):
    keep = []

    def z(n, v=0.0):      # (kept alive: the calls take addresses)
        keep.append(np.full(n, v))
        return keep[-1]
    for n_col, E in ((20, 4), (20, 2)):
        nx, nf, k = 9 * (n_col + 1), 3 * E * n_col, 3 * E
        for first in ("band", "blocks"):
            h = hiplib.bmpc_biconvex_create(2.5, n_col, E)
            try:
                calls = [lambda: hiplib.bmpc_biconvex_set_cost_x_band(h, z(nx, 1.0).ctypes.data, z(9 * n_col).ctypes.data, z(nx).ctypes.data),
                         lambda: hiplib.bmpc_biconvex_set_cost_f_blocks(h, z(k * k * n_col).ctypes.data, z(nf).ctypes.data)]
                for call in (calls if first == "band" else calls[::-1]):
                    assert call() == _lib.OK
                assert hiplib.bmpc_biconvex_optimize(h, z(9).ctypes.data, 1) == _lib.BAD_ARG
                msg = hiplib.bmpc_last_error().decode()
                assert "neighbouring knots" in msg and "blocks" in msg, msg
                # the diagonal setter returns the side to its diagonal: the refusal is gone (what is missing now is the contact plan)
                assert hiplib.bmpc_biconvex_set_cost_x(h, z(nx, 1.0).ctypes.data, z(nx).ctypes.data) == _lib.OK
                assert hiplib.bmpc_biconvex_optimize(h, z(9).ctypes.data, 1) != _lib.OK
                assert "neighbouring knots" not in hiplib.bmpc_last_error().decode()
            finally:
                hiplib.bmpc_biconvex_destroy(h)
    # the handle's horizon limit: 64 knots
    h = hiplib.bmpc_biconvex_create(2.5, 64, 4)
    try:
        assert hiplib.bmpc_biconvex_set_cost_f_band(h, z(12 * 64, 1.0).ctypes.data, z(12 * 63).ctypes.data, z(12 * 64).ctypes.data) == _lib.OK
        assert hiplib.bmpc_biconvex_optimize(h, z(9).ctypes.data, 1) == _lib.BAD_ARG
        assert "64 knots" in hiplib.bmpc_last_error().decode()
        assert hiplib.bmpc_biconvex_set_cost_x_band(None, None, None, None) == _lib.BAD_ARG
    finally:
        hiplib.bmpc_biconvex_destroy(h)


def test_batch_wrappers_refuse_bad_shapes_and_blocks_with_coupling(oracle):
    from bunmpc_amd import batch as bb
    b = problems.make_batch("solo12_trot", 2, H=5)
    pre = oracle.solve_batch(b, num_iters=0)
    raw = {k: pre[k] for k in ("Qx", "qx", "lbx", "ubx", "Qf")}
    with pytest.raises(ValueError, match="Qx_off"):
        bb.solve_host(b, raw=dict(raw, Qx_off=np.zeros((2, 6, 9))))
    with pytest.raises(ValueError, match="Qf_off"):
        bb.solve_host(b, raw=dict(raw, Qf_off=np.zeros((3, 4, 12))))
    with pytest.raises(ValueError, match="per-knot blocks"):
        bb.solve_host(b, raw=dict(raw, Qf_off=np.zeros((1, 4, 12)), Qx_blk=np.zeros((1, 6, 9, 9))))
