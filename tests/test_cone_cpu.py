"""The Euclidean friction-cone projection without a GPU: the projection's defining properties (and the reference step's failure of one
of them, the reason for the mode), the numpy twin on the Go2 and mixed-gait problems the reference's projection cannot solve
deterministically, the precondition of the GPU cases (the twin does not move under a one-ulp change of its input), and the C-ABI's
refusals and bindings."""
import ctypes as C

import numpy as np
import pytest

from bunmpc_amd import _lib, problems
from bunmpc_amd import batch as bb
from bunmpc_amd.biconvex_mpc_cpp import BiconvexMP
from oracle import oracle_np
from tests import cone_np
from tests.util import MAPPINGS, rel_l2, restatement


def _draws():
    """10^4 vectors and coefficients, some exactly on the axis, on the cone's surface, on the polar cone's surface and at the origin"""
    rng = np.random.default_rng(20251017)
    n = 10000
    v = rng.normal(0.0, 3.0, size=(n, 3))
    mu = rng.uniform(0.05, 2.0, size=n)
    mu[:50] = 1.0
    v[0:10, 0:2] = 0.0                                           # the axis, both directions
    v[10:20] = 0.0                                               # the origin
    v[20:30, 2] = np.hypot(v[20:30, 0], v[20:30, 1])             # the cone's surface at mu = 1 (to rounding)
    v[30:40, 2] = -np.hypot(v[30:40, 0], v[30:40, 1])            # the polar cone's
    v[40:45] = [3.0, 4.0, 5.0]                                   # ... exactly: |f_xy| = 5 = fz
    v[45:50] = [3.0, 4.0, -5.0]
    return v, mu


def test_projection_is_the_euclidean_projection():
    v, mu = _draws()
    count = [0, 0, 0]
    p = cone_np.project(v, mu, count)
    assert sum(count) == len(v) and min(count) > 1000
    assert np.array_equal(p[10:20], np.zeros((10, 3))) and np.array_equal(p[40:45], v[40:45]) and np.array_equal(p[45:50], np.zeros((5, 3)))
    assert np.array_equal(p[0:10, 0:2], np.zeros((10, 2))) and np.array_equal(p[0:10, 2], np.maximum(v[0:10, 2], 0.0))
    scale = 1.0 + np.linalg.norm(v, axis=1)
    # feasible
    assert np.all(p[:, 2] >= 0)
    assert np.all(np.hypot(p[:, 0], p[:, 1]) - mu * p[:, 2] <= 1e-14 * scale)
    # idempotent
    assert np.all(np.linalg.norm(cone_np.project(p, mu) - p, axis=1) <= 1e-14 * scale)
    # v - P(v) lies in the polar cone {w: wz <= 0, mu |w_xy| <= -wz} and is orthogonal to P(v)
    w = v - p
    assert np.all(w[:, 2] <= 1e-14 * scale) and np.all(mu * np.hypot(w[:, 0], w[:, 1]) + w[:, 2] <= 1e-14 * scale)
    assert np.all(np.abs(np.sum(w * p, axis=1)) <= 1e-13 * scale * scale)
    # non-expansive, pairs with the same coefficient
    a, b, m = v[0::2], v[1::2], np.repeat(mu[0::2, None], 1, axis=1).reshape(-1)
    pa, pb = cone_np.project(a, m), cone_np.project(b, m)
    assert np.all(np.linalg.norm(pa - pb, axis=1) <= np.linalg.norm(a - b, axis=1) * (1 + 1e-12))


def test_reference_step_is_expansive_on_the_same_draws():
    """fista.cpp:52-70 is no projection: on the same pairs it moves points apart"""
    v, mu = _draws()
    a, b, m = v[0::2], v[1::2], mu[0::2]
    pa = np.stack([oracle_np.soc_projection(a[i], m[i]) for i in range(len(a))])
    pb = np.stack([oracle_np.soc_projection(b[i], m[i]) for i in range(len(a))])
    grew = np.linalg.norm(pa - pb, axis=1) > np.linalg.norm(a - b, axis=1) * (1 + 1e-12)
    with np.errstate(invalid="ignore"):      # (the pairs of identical points: 0 / 0)
        print("expansive on", int(grew.sum()), "of", len(a), "pairs, worst ratio", np.nanmax(np.linalg.norm(pa - pb, axis=1) / np.linalg.norm(a - b, axis=1)))
    assert grew.sum() > 0


def test_go2_at_mu_one():
    """go2_bound, H = 40, mu = 1, cold, 10 ADMM iterations: the reference's projection overflows to NaN in the first ADMM iteration, the
    Euclidean projection solves every problem (ten iterations, violation 1.08 .. 1.10: the cold start's ten iterations do not converge
    under either projection -- the reference's at mu = 10 leaves the same violation)"""
    b = problems.make_batch("go2_bound", 4, H=40)
    raw = cone_np.raw_batch(b)
    for i in range(4):
        ref = restatement(b, i, raw, 10, mu=1.0)
        assert ref["stats"][5] == 2 and ref["stats"][0] == 1, ref["stats"]
        r = cone_np.restatement(b, i, 10, 1.0)
        print("go2", i, "reference", ref["stats"].tolist(), "euclidean", r["stats"].tolist(), "violation", r["hist"][-1])
        assert r["stats"][5] == 0 and r["stats"][0] == 10 and 1.08 <= round(r["hist"][-1], 2) <= 1.10


def test_mixed_gaits_become_deterministic():
    """solo12_mixed, mu = 0.5, problem 2, cold, 10 iterations: one ulp of x_init[0] changes the reference projection's counts and moves
    its forces by 1e-3; under the Euclidean projection the counts stay and the forces move by rounding -- in fewer force iterations"""
    b = problems.make_batch("solo12_mixed", 3)
    x1 = cone_np.one_ulp(b.x_init[2])
    ref, ref1 = (restatement(b, 2, cone_np.raw_batch(b), 10, mu=0.5, x_init=x) for x in (None, x1))
    r, r1 = (cone_np.restatement(b, 2, 10, 0.5, x_init=x) for x in (None, x1))
    print("reference", ref["stats"].tolist(), ref1["stats"].tolist(), rel_l2(ref1["F"], ref["F"]), "euclidean", r["stats"].tolist(), r1["stats"].tolist(), rel_l2(r1["F"], r["F"]))
    assert not np.array_equal(ref["stats"], ref1["stats"]) and rel_l2(ref1["F"], ref["F"]) > 1e-4
    assert np.array_equal(r["stats"], r1["stats"]) and rel_l2(r1["F"], r["F"]) < 1e-12
    assert r["stats"][5] == 0 and r["stats"][1] < ref["stats"][1]


@pytest.mark.parametrize("H,lanes", MAPPINGS)
@pytest.mark.parametrize("config", cone_np.CONFIGS)
def test_gpu_cases_are_well_posed(config, H, lanes):
    """the precondition of tests/test_cone_gpu.py: per problem the twin and the twin with x_init[0] moved by one ulp agree on every
    count and on X / F / P to 1e-12; per case all three branches of the projection are taken and the force loop retries"""
    base, moved = cone_np.twin(config, H), cone_np.twin(config, H, perturbed=True)
    for i, (r, r1) in enumerate(zip(base, moved)):
        assert np.array_equal(r["stats"], r1["stats"]) and r["L_f"] == r1["L_f"] and r["L_x"] == r1["L_x"], i
        assert r["stats"][5] == 0
        for k in "XFP":
            assert rel_l2(r1[k], r[k]) < 1e-12, (i, k)
    branches = np.sum([r["branches"] for r in base], axis=0)
    print(config, H, "branches", branches.tolist(), "force retries", [int(r["stats"][3]) for r in base])
    assert np.all(branches > 0)
    assert sum(r["stats"][3] for r in base) >= 1


# ---- the C-ABI without a GPU: every refusal comes before the first HIP call -----------------------------------------------------------

def _host(b, cone, **kw):
    with pytest.raises(_lib.BmpcError) as e:
        bb.solve_host(b, num_iters=1, cone=cone, **kw)
    assert e.value.code == _lib.BAD_ARG
    return str(e.value)


def test_batch_refusals():
    b = problems.make_batch("solo12_trot", 2, H=20)
    mu = np.full((2, 20, 4), 0.2)
    assert "projection = 1" in _host(b, dict(projection="reference", mu=mu))
    assert "fp64" in _host(b, dict(projection="euclidean"), precision="f32")
    assert "64 knots" in _host(problems.make_batch("solo12_trot", 2, H=64), dict(projection="euclidean"))
    for bad in (0.0, -0.1, np.nan, np.inf):
        m = mu.copy()
        m[1, 7, 2] = bad
        assert "finite and > 0" in _host(b, dict(projection="euclidean", mu=m))
    assert "finite and > 0" in _host(b, dict(projection="euclidean"), mu=0.0)
    with pytest.raises(ValueError):
        bb.solve_host(b, cone=dict(projection="euclidean", mu=np.full((2, 20, 3), 0.2)))
    with pytest.raises(ValueError):
        bb.solve_host(b, cone=dict(projection="conic"))
    raw = cone_np.raw_batch(b)
    with pytest.raises(ValueError):
        bb.solve_host(b, raw=dict(raw, Qf_off=np.zeros((1, 19, 12))), cone=dict(projection="euclidean"))
    # straight to the C call: a projection that does not exist, strides, n_eff
    lib = _lib.lib()
    d = _lib.Batch()
    lib.bmpc_batch_defaults(C.byref(d))
    d.B, d.n_col, d.n_eff = 2, 20, 4
    flat = np.ascontiguousarray(mu)
    for cone, word in ((_lib.Cone(projection=2), "projection must be"), (_lib.Cone(projection=1, mu=flat.ctypes.data, smu=79), "smu"),
                       (_lib.Cone(projection=1, mu=flat.ctypes.data, smu=-1), "smu"), (_lib.Cone(projection=1, mu=flat.ctypes.data, smu=(1 << 26) + 1), "smu")):
        for fn in (lambda c: lib.bmpc_biconvex_solve_batch_cone_host(C.byref(d), C.byref(c)), lambda c: lib.bmpc_biconvex_solve_batch_cone_device(C.byref(d), C.byref(c), None)):
            assert fn(cone) == _lib.BAD_ARG and word in _lib.last_error(), (word, _lib.last_error())
    d.n_eff = 3
    assert lib.bmpc_biconvex_solve_batch_cone_host(C.byref(d), C.byref(_lib.Cone(projection=1))) == _lib.BAD_ARG and "n_eff" in _lib.last_error()


def test_handle_refusals():
    b = problems.make_batch("solo12_trot", 1, H=20)
    mp = BiconvexMP(b.m, 20, 4)
    for t in range(20):
        mp.set_contact_plan(b.cnt_plan[0, t], b.dt[0, t])
    with pytest.raises(ValueError):
        mp.set_cone_projection("conic")
    with pytest.raises(ValueError):
        mp.set_friction_coefficients(np.ones(3))
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(_lib.BmpcError) as e:
            mp.set_friction_coefficients(np.array([0.2, 0.2, bad, 0.2]))
        assert e.value.code == _lib.BAD_ARG and "finite and > 0" in str(e.value)
    assert mp._lib.bmpc_biconvex_set_cone_projection(mp._h, 2) == _lib.BAD_ARG
    # an array under the reference's projection
    mp.set_friction_coefficients(np.full((20, 4), 0.2))
    with pytest.raises(_lib.BmpcError) as e:
        mp.optimize(b.x_init[0], 1)
    assert e.value.code == _lib.BAD_ARG and "set_cone_projection" in str(e.value)
    # block and band costs under the Euclidean projection
    mp.set_cone_projection("euclidean")
    r = cone_np.raw_of(b, 0)
    blk = np.diag(r["Qf"])
    blk[0, 1] = blk[1, 0] = 1e-5
    mp.set_cost_f(blk, np.zeros(mp.nf))
    with pytest.raises(_lib.BmpcError) as e:
        mp.optimize(b.x_init[0], 1)
    assert e.value.code == _lib.BAD_ARG and "diagonal costs only" in str(e.value)
    band = np.diag(r["Qx"]) + np.diag(np.full(mp.nx - 9, 0.5), 9) + np.diag(np.full(mp.nx - 9, 0.5), -9)
    mp.set_cost_f(r["Qf"], np.zeros(mp.nf))
    mp.set_cost_x(band, r["qx"])
    with pytest.raises(_lib.BmpcError) as e:
        mp.optimize(b.x_init[0], 1)
    assert e.value.code == _lib.BAD_ARG and "diagonal costs only" in str(e.value)
    # more than 64 knots
    big = problems.make_batch("solo12_trot", 1, H=64)
    mp = BiconvexMP(big.m, 64, 4)
    for t in range(64):
        mp.set_contact_plan(big.cnt_plan[0, t], big.dt[0, t])
    mp.set_cone_projection("euclidean")
    with pytest.raises(_lib.BmpcError) as e:
        mp.optimize(big.x_init[0], 1)
    assert e.value.code == _lib.BAD_ARG and "64 knots" in str(e.value)


_I, _P = C.c_int, C.c_void_p
_CONE = {"bmpc_cone_struct_size": (_I, []),
         "bmpc_biconvex_solve_batch_cone_device": (_I, [_P, _P, _P]),
         "bmpc_biconvex_solve_batch_cone_host": (_I, [_P, _P]),
         "bmpc_biconvex_set_cone_projection": (_I, [_P, _I]),
         "bmpc_biconvex_set_friction_coefficients": (_I, [_P, _P]),
         "bmpc_biconvex_cone_kernel_scratch_bytes": (_I, [_I])}


def test_cone_bindings_match_the_header(hiplib):
    """the cone entry points' signatures as the binding reads them from include/bunmpc.h (tests/test_abi_cpu.py holds the whole table),
    the struct's size, the minor version"""
    for name, sig in _CONE.items():
        assert _lib._SIGS[name] == sig, name
    assert hiplib.bmpc_cone_struct_size() == C.sizeof(_lib.Cone) == 24
    assert hiplib.bmpc_abi_minor_version() == 2
    assert hiplib.bmpc_biconvex_cone_kernel_scratch_bytes(3) == -1
