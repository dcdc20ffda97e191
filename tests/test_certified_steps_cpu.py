"""The numpy restatement of the step certificate's bound (tools/certify_rate.py; the kernel's in biconvex_admm_body.h) against the
largest eigenvalue of the dense Hessians Q + rho A'A: on workload problems (cold and after a few ADMM iterations) and on random
block structures with adversarial scales."""
import os
import sys

import numpy as np
import pytest

from bunmpc_amd import problems

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import certify_rate as cr  # noqa: E402


def _check(oracle, cnt, dt, m, X, F, W_F, Qx, x_init, rho):
    B = cnt.shape[0]
    lf, df = cr.force_bound_terms(cnt, dt, m, X, W_F, rho)
    lm, dm = cr.motion_bound_terms(cnt, dt, F, Qx, rho)
    bf, bm = cr.bound_from_terms(lf, df), cr.bound_from_terms(lm, dm)
    for i in range(B):
        A, _ = oracle.dense_A_x(cnt[i], dt[i], m, X[i])
        Mf = np.diag(W_F[i]) + rho * A.T @ A
        assert np.allclose(np.diag(Mf), df[i].ravel(), rtol=1e-12)
        assert bf[i] >= np.linalg.eigvalsh(Mf).max() * (1 - 1e-12)
        Af, _ = oracle.dense_A_f(cnt[i], dt[i], m, F[i], x_init[i])
        Mx = np.diag(Qx[i]) + rho * Af.T @ Af
        assert np.allclose(np.diag(Mx), dm[i].ravel(), rtol=1e-12)
        assert bm[i] >= np.linalg.eigvalsh(Mx).max() * (1 - 1e-12)


@pytest.mark.parametrize("config", ["solo12_trot", "solo12_mixed", "go2_bound", "biped_walk"])
def test_bound_covers_workload_hessians(oracle, config):
    b = problems.make_batch(config, 12)
    Qx, W_F = cr._costs(b)
    X0, F0, _ = b.warm_start()
    o = oracle.solve_batch(b, num_iters=3, fast=True)
    for X, F in ((X0, F0), (X0, o["F"]), (o["X"], o["F"])):
        _check(oracle, b.cnt_plan, b.dt, b.m, X, F, W_F, Qx, b.x_init, b.rho)


@pytest.mark.parametrize("seed", range(6))
def test_bound_covers_random_block_structures(oracle, seed):
    """random contact flags, foot positions, step lengths, forces and weights over many orders of magnitude"""
    rng = np.random.default_rng(seed)
    B, H, E = 4, int(rng.integers(1, 12)), (2, 4)[seed % 2]
    cnt = np.zeros((B, H, E, 4))
    cnt[..., 0] = rng.integers(0, 2, (B, H, E))
    cnt[..., 1:4] = rng.normal(0.0, 10.0 ** rng.uniform(-2, 1), (B, H, E, 3))
    dt = 10.0 ** rng.uniform(-3, 0, (B, H))
    m = float(10.0 ** rng.uniform(-1, 2))
    X = rng.normal(0.0, 10.0 ** rng.uniform(-2, 1), (B, 9 * (H + 1)))
    F = rng.normal(0.0, 10.0 ** rng.uniform(-1, 3), (B, 3 * E * H))
    W_F = 10.0 ** rng.uniform(-6, 3, (B, 3 * E * H))
    Qx = 10.0 ** rng.uniform(-6, 7, (B, 9 * (H + 1)))
    x_init = rng.normal(0.0, 1.0, (B, 9))
    rho = float(10.0 ** rng.uniform(-2, 5))
    _check(oracle, cnt, dt, m, X, F, W_F, Qx, x_init, rho)


def test_certificate_rate_on_the_headline_workload():
    """the certificate holds for every phase of the bench's problems (sampled): the premise of the certified loops' gain"""
    r = cr.rates(problems.make_batch("solo12_trot", 64), num_iters=10)
    assert r["force"] == 1.0 and r["motion"] == 1.0
