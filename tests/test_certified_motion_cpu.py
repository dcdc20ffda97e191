"""The motion step's certificate (tools/certify_rate.py: motion_bound_terms; the kernel's in biconvex_admm_body.h) at the corners
tests/test_certified_steps_cpu.py does not reach -- one knot interval, zero forces (S = 0), zero weights -- against the largest
eigenvalue of the dense Hessian, and the phase-by-phase prediction tests/test_certified_motion_gpu.py holds the kernel's telemetry to."""
import os
import sys

import numpy as np
import pytest

from bunmpc_amd import problems

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import certify_rate as cr  # noqa: E402


@pytest.mark.parametrize("seed", range(50))
def test_certified_problems_have_their_eigenvalues_below_half_L(oracle, seed):
    """random block-tridiagonal structures of the motion step's shape: whatever the certificate passes has lambda_max(M) <= L/2"""
    rng = np.random.default_rng(1000 + seed)
    B, E = 4, (2, 4)[seed % 2]
    H = (1, 2, 31)[seed] if seed < 3 else int(rng.integers(1, 32))
    cnt = np.zeros((B, H, E, 4))
    cnt[..., 0] = rng.integers(0, 2, (B, H, E))
    cnt[..., 1:4] = rng.normal(0.0, 1.0, (B, H, E, 3))
    dt = 10.0 ** rng.uniform(-3, 0, (B, H))
    m = float(10.0 ** rng.uniform(-1, 2))
    F = rng.normal(0.0, 10.0 ** rng.uniform(-1, 3), (B, 3 * E * H))
    F[0] = 0.0                                                   # S = 0 on every knot
    F[1].reshape(H, 3 * E)[rng.integers(0, 2, H) == 0] = 0.0     # ... on some
    Qx = 10.0 ** rng.uniform(-6, 7, (B, 9 * (H + 1)))
    Qx[2] = 0.0                                                  # no weight at all
    Qx[3][rng.integers(0, 2, 9 * (H + 1)) == 0] = 0.0            # ... on some components
    x_init = rng.normal(0.0, 1.0, (B, 9))
    rho = float(10.0 ** rng.uniform(-2, 5))
    lhs, dg = cr.motion_bound_terms(cnt, dt, F, Qx, rho)
    bound = cr.bound_from_terms(lhs, dg)
    # step constants on both sides of the certificate's threshold bound <= (L/2)(1 - eta)
    L = 2.0 * bound / (1.0 - cr.ETA) * np.array([0.5, 0.999, 1.001, 4.0])[(np.arange(B) + seed) % 4]
    ok = cr.certified(lhs, dg, L)
    assert np.array_equal(ok, bound <= 0.5 * L * (1.0 - cr.ETA))
    for i in range(B):
        Af, _ = oracle.dense_A_f(cnt[i], dt[i], m, F[i], x_init[i])
        Mx = np.diag(Qx[i]) + rho * Af.T @ Af
        assert np.allclose(np.diag(Mx), dg[i].ravel(), rtol=1e-12)
        if ok[i]:
            assert np.linalg.eigvalsh(Mx).max() <= 0.5 * L[i]
    assert ok.any() and not ok.all()


def test_phase_predictions_of_the_small_step_constant_case(oracle):
    """the case of tests/test_certified_motion_gpu.py::test_small_step_constants: no phase lies within 1e-9 of its threshold (the GPU
    test may leave out one in ten), the problems with the small L_x fail their first motion phase, and so do their wave-mates"""
    B, K = 6, 5
    b = problems.make_batch("solo12_trot", B)
    Lx = np.where(np.arange(B) % 3 == 0, 1e4, 2.25e6)
    pred = cr.phase_predictions(b, oracle, K, warm=b.warm_start(), L_x=Lx)
    assert pred["ran"].all()
    for which in ("force", "motion"):
        _, usable = cr.wave_phases(pred, which)
        assert (pred["ran"] & ~usable).sum() * 10 <= pred["ran"].sum()
        assert pred[which + "_gap"].min() > 1e-3
    assert np.array_equal(pred["motion"][:, 0], np.arange(B) % 3 != 0) and pred["motion"][:, 1:].all() and pred["force"].all()
    want, _ = cr.wave_phases(pred, "motion")
    assert np.array_equal(want[:, 0], np.arange(B) >= 4)
