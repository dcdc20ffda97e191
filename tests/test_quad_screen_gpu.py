"""The quad stage of the certified loops' screen on the device (biconvex_lanes.h: quad_sum_f32, quad_theta_f32, quad_screen) against its
numpy model (tests/quad_screen_np.py), bit for bit and lane for lane: the margin proof of tests/test_quad_screen_cpu.py argues about the
model, and this is what makes it a statement about the hardware -- the order of the conversion and the two DPP additions, the rounding
of float(theta (1 + 2^-20)), its floor of 2^-100, subnormal, NaN and infinite operands.  The probe is a kernel of its own in
csrc/lane_probe.hip behind a test-only entry point that no header declares (the headers' tables and the seven groups of
bmpc_probe_lanes are held to their recorded sizes by tests/test_abi_cpu.py and tests/test_lane_probe_cpu.py): bound here by name.
A wave of 64 lanes is one test case: in [waves][2][64] (g2, theta as doubles), out [waves][3][64] (the quad sum and the threshold as
floats in the low halves, the ballot of quad_screen)."""
import ctypes as C

import numpy as np
import pytest

from bunmpc_amd import _lib
from tests import quad_screen_np as qs

pytestmark = pytest.mark.gpu

U64, U32 = np.uint64, np.uint32


def probe(hiplib, g2, theta):
    """g2, theta [waves][64] doubles -> (quad sums [waves][64] float32, thresholds [waves][64] float32, ballots [waves] uint64)"""
    fn = hiplib.bmpc_probe_quad_screen
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    rows = np.ascontiguousarray(np.stack([np.asarray(g2, np.float64), np.asarray(theta, np.float64)], axis=1)).view(U64)
    out = np.full((rows.shape[0], 3, 64), 0xdeadbeefdeadbeef, U64)
    assert fn(rows.ctypes.data, rows.nbytes, out.ctypes.data, out.nbytes) == _lib.OK
    assert np.all(out[:, :2] >> U64(32) == 0) and np.all(out[:, 2] == out[:, 2, :1]), "floats in the low halves, one ballot per wave"
    return out[:, 0].astype(U32).view(np.float32), out[:, 1].astype(U32).view(np.float32), out[:, 2, 0]


def model(g2, theta):
    with np.errstate(invalid="ignore"):
        q, th = qs.quad_sum(g2), qs.quad_theta(theta)
        ballot = ((q > th).astype(U64) << np.arange(64, dtype=U64)).sum(axis=1, dtype=U64)
    return q, th, ballot


def check(hiplib, g2, theta):
    g2, theta = np.asarray(g2, np.float64), np.broadcast_to(np.asarray(theta, np.float64), np.shape(g2))
    q, th, ballot = probe(hiplib, g2, theta)
    mq, mth, mballot = model(g2, theta)
    assert np.array_equal(q.view(U32), mq.view(U32)), "quad_sum_f32"
    assert np.array_equal(th.view(U32), mth.view(U32)), "quad_theta_f32"
    assert np.array_equal(ballot, mballot), "quad_screen"
    return int(np.count_nonzero(mq > mth))


def test_bad_arguments_are_refused():
    fn = _lib.lib().bmpc_probe_quad_screen
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long]
    buf = (C.c_ulonglong * (64 * 3 * 2))()
    for args in ((None, 1024, buf, 1536), (buf, 1024, None, 1536), (buf, 0, buf, 0), (buf, 1032, buf, 1536), (buf, 1024, buf, 1528), (buf, 2048, buf, 1536)):
        assert fn(*args) == _lib.BAD_ARG, args[1::2]


def test_random_partials_and_thresholds(hiplib):
    rng = np.random.default_rng(1)
    theta = 10.0 ** rng.uniform(-40, 38, (200, 1))
    g2 = theta * 10.0 ** rng.uniform(-3, 1, (200, 64)) * rng.random((200, 64)) ** rng.integers(1, 6, (200, 1))
    g2[:, 21:32] = 0.0      # (a 21-knot segment: the lanes without a knot hold zeros)
    fired = check(hiplib, g2, theta)
    assert 1000 < fired < 200 * 64 - 1000


@pytest.mark.parametrize("shape", ["equal", "dominant", "two", "ramp"])
def test_quads_at_the_threshold(hiplib, shape):
    """the adversarial quads of tests/test_quad_screen_cpu.py: sums within a few fp32 ulps of the threshold on either side, every
    partial stepped by single fp64 ulps (the conversion's ties); sixteen quads per wave"""
    rng = np.random.default_rng(2)
    w = np.array({"equal": [0.25, 0.25, 0.25, 0.25], "dominant": [1 - 3e-9, 1e-9, 1e-9, 1e-9], "two": [0.5, 0.5, 0.0, 0.0], "ramp": [0.1, 0.2, 0.3, 0.4]}[shape])
    g2, th = [], []
    for theta in (1e-10 * (1.0 + 2.0 ** -40), 1e-6, 9e-8, 2.0 ** -100, 2.0 ** -126, 1e30, 3e38, 10.0 ** -23.5):
        thq = float(qs.quad_theta(theta))
        rel = np.concatenate([np.linspace(-8, 8, 65) * 2.0 ** -24, rng.uniform(-1, 1, 63) * 2.0 ** -20])      # 128 quads: 8 waves
        base = w[None, :] * thq * (1.0 + rel[:, None])
        for _ in range(8):
            g2.append(base.reshape(8, 64).copy())
            th.append(np.full((8, 64), theta))
            base = np.nextafter(base, np.inf)
    fired = check(hiplib, np.concatenate(g2), np.concatenate(th))
    assert fired > 1000


def test_subnormals_zeros_nan_inf_and_the_switch(hiplib):
    rng = np.random.default_rng(3)
    tiny = 2.0 ** rng.uniform(-160, -120, (40, 64))      # subnormal in fp32, and the smallest normals beside them
    tiny[::3, 1::4] = 0.0
    tiny[1::3, 0::4] = 2.0 ** rng.uniform(-101, -99, tiny[1::3, 0::4].shape)      # one normal lane per quad around the threshold's floor
    for theta in (2.0 ** -1000, 2.0 ** -200, 2.0 ** -140, 2.0 ** -126, 2.0 ** -101, 2.0 ** -100):
        check(hiplib, tiny, theta)
    g = rng.random((8, 64))
    g[0, 5] = np.nan
    g[1, 63] = np.inf
    g[2, ::4] = 1e39      # (overflows fp32: +inf, above every finite threshold)
    g[3, 17] = -np.nan
    g[4, :] = 0.0
    th = np.full((8, 64), 1e-10)
    th[5] = np.inf        # the screen switched off: nothing settles
    th[6] = 3.5e38        # the threshold itself overflows fp32
    th[7] = 3.4e38
    g[7, 8:12] = 1e39
    fired = check(hiplib, g, th)
    assert fired > 0
    q, t, ballot = probe(hiplib, g, th)
    assert ballot[5] == 0 and ballot[6] == 0 and np.isinf(t[5]).all() and np.isinf(t[6]).all()
    assert ballot[0] == 0xffffffffffffffff & ~(0xf << 4), "a NaN partial settles nothing in its own quad and changes nothing in the next"
    assert ballot[7] == 0xf << 8
