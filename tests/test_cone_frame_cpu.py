"""Friction cones about per-contact surface normals without a GPU: the projection's defining properties in a tilted frame and its
equivariance with the world-z projection, the precondition of the GPU cases (the twin does not move under a one-ulp change of its
input), a slope on which world-z cones slip and the plane's normals do not, and the C-ABI's refusals and bindings.

Bounds.  A projected vector and each quantity a property is read from (n.f, f - (n.f) n, its norm) come out of at most a dozen
operations on numbers no larger than (1 + mu) |v| <= 3 |v|, each with a relative rounding of 1.1e-16: 1e-14 (1 + |v|), the world-z
tests' own bound, covers both sides of a comparison; products of two such vectors are held to 1e-13 (1 + |v|)^2, as there."""
import ctypes as C
import os

import numpy as np
import pytest

from bunmpc_amd import _lib, problems
from bunmpc_amd import batch as bb
from bunmpc_amd.biconvex_mpc_cpp import BiconvexMP
from tests import cone_frame_np, cone_np
from tests.test_cone_cpu import _draws
from tests.util import MAPPINGS, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUCLID = dict(projection="euclidean")


def _rotations(n, seed):
    """n rotation matrices from unit quaternions drawn uniformly: (n, 3, 3), each orthogonal to rounding, determinant +1"""
    q = np.random.default_rng(seed).normal(size=(n, 4))
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=-1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=-1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1)], axis=1)


def test_projection_is_the_euclidean_projection_in_a_tilted_frame():
    v0, mu = _draws()
    R = _rotations(len(v0), 20251018)
    v = np.einsum("nij,nj->ni", R, v0)
    n = np.ascontiguousarray(R[:, :, 2])      # R e3
    assert np.abs(np.sum(n * n, axis=1) - 1.0).max() <= 1e-9
    count = [0, 0, 0]
    p = cone_frame_np.project_frame(v, mu, n, count)
    print("branches", count)
    assert sum(count) == len(v) and min(count) > 1000
    scale = 1.0 + np.linalg.norm(v, axis=1)
    # feasible in the tilted cone
    fn, excess = cone_frame_np.cone_excess(p, mu, n)
    print("feasible: min fn / scale", (fn / scale).min(), "worst excess / scale", (excess / scale).max())
    assert np.all(fn >= -1e-14 * scale) and np.all(excess <= 1e-14 * scale)
    # idempotent
    again = np.linalg.norm(cone_frame_np.project_frame(p, mu, n) - p, axis=1)
    print("idempotent", (again / scale).max())
    assert np.all(again <= 1e-14 * scale)
    # v - P(v) lies in the polar cone {w: n.w <= 0, mu |w_t| <= -n.w} and is orthogonal to P(v)
    w = v - p
    wn = np.sum(w * n, axis=1)
    wt = np.linalg.norm(w - wn[:, None] * n, axis=1)
    print("polar", (wn / scale).max(), ((mu * wt + wn) / scale).max(), "orthogonal", (np.abs(np.sum(w * p, axis=1)) / scale ** 2).max())
    assert np.all(wn <= 1e-14 * scale) and np.all(mu * wt + wn <= 1e-14 * scale)
    assert np.all(np.abs(np.sum(w * p, axis=1)) <= 1e-13 * scale * scale)
    # non-expansive: pairs with the same coefficient and the same normal
    a, b, m, na = v[0::2], np.einsum("nij,nj->ni", R[0::2], v0[1::2]), mu[0::2], n[0::2]
    pa, pb = cone_frame_np.project_frame(a, m, na), cone_frame_np.project_frame(b, m, na)
    assert np.all(np.linalg.norm(pa - pb, axis=1) <= np.linalg.norm(a - b, axis=1) * (1 + 1e-12))
    # equivariant: P_n(R v) = R P_z(v) for n = R e3
    want = np.einsum("nij,nj->ni", R, cone_np.project(v0, mu))
    err = np.linalg.norm(p - want, axis=1)
    print("equivariance", (err / (1.0 + np.linalg.norm(v0, axis=1))).max())
    assert np.all(err <= 1e-14 * (1.0 + np.linalg.norm(v0, axis=1)))
    # the world-z normal: cone_np.project's values, branch by branch
    cz = [0, 0, 0]
    pz = cone_frame_np.project_frame(v0, mu, np.array([0.0, 0.0, 1.0]), cz)
    c0 = [0, 0, 0]
    assert np.array_equal(pz, cone_np.project(v0, mu, c0)) and cz == c0
    # inside the cone: the input's bits
    inside = (fn0 := np.sum(v * n, axis=1)) > 0
    inside &= np.linalg.norm(v - fn0[:, None] * n, axis=1) < 0.5 * mu * fn0
    assert inside.sum() > 100 and np.array_equal(p[inside].view(np.uint64), v[inside].view(np.uint64))


@pytest.mark.parametrize("H,lanes", MAPPINGS)
@pytest.mark.parametrize("config", cone_np.CONFIGS)
def test_gpu_cases_are_well_posed(config, H, lanes):
    """the precondition of tests/test_cone_frame_gpu.py: per problem the twin and the twin with x_init[0] moved by one ulp agree on
    every count and step constant and on X / F / P to 1e-12, status 0; per case all three branches of the projection are taken and
    the force loop retries.  No problem is left out."""
    base, moved = cone_frame_np.twin(config, H), cone_frame_np.twin(config, H, perturbed=True)
    for i, (r, r1) in enumerate(zip(base, moved)):
        assert np.array_equal(r["stats"], r1["stats"]) and r["L_f"] == r1["L_f"] and r["L_x"] == r1["L_x"], i
        assert r["stats"][5] == 0
        for k in "XFP":
            assert rel_l2(r1[k], r[k]) < 1e-12, (i, k)
    branches = np.sum([r["branches"] for r in base], axis=0)
    print(config, H, "branches", branches.tolist(), "force retries", [int(r["stats"][3]) for r in base],
          "one-ulp spread", max(rel_l2(r1[k], r[k]) for r, r1 in zip(base, moved) for k in "XFP"))
    assert np.all(branches > 0)
    assert sum(r["stats"][3] for r in base) >= 1


def test_world_z_cones_slip_on_a_slope():
    """one trot problem on a plane pitched by 25 degrees, mu = 0.3 (atan(mu) = 16.7 degrees): the forces of the world-z solve leave the
    plane's friction cone, the forces of the solve with the plane's normals lie in it to 1e-12"""
    mu, pitch = 0.3, np.deg2rad(25.0)
    assert np.tan(pitch) > mu
    b = problems.make_batch("solo12_trot", 1, H=15)
    nrm = problems.plane_normals(1, b.H, b.E, 0.0, pitch)
    assert nrm.shape == (1, b.H, b.E, 3) and np.abs(np.sum(nrm * nrm, axis=-1) - 1.0).max() <= 1e-15
    assert np.allclose(nrm[0, 0, 0], [np.sin(pitch), 0.0, np.cos(pitch)])
    flat = cone_np.restatement(b, 0, 3, mu)
    tilt = cone_frame_np.restatement(b, 0, 3, mu, nrm[0])
    assert flat["stats"][5] == 0 and tilt["stats"][5] == 0
    fn, ex = cone_frame_np.cone_excess(flat["F"], mu, nrm[0])
    print("world-z cones on the slope: worst |ft| - mu fn", ex.max(), "of forces up to", np.abs(flat["F"]).max())
    assert ex.max() > 1e-3
    fn, ex = cone_frame_np.cone_excess(tilt["F"], mu, nrm[0])
    print("the plane's normals: min fn", fn.min(), "worst |ft| - mu fn", ex.max(), "branches", tilt["branches"].tolist())
    assert np.any(fn > 1e-3) and fn.min() >= -1e-12 and ex.max() <= 1e-12
    assert tilt["branches"][2] > 0


def test_plane_normals_per_problem():
    n = problems.plane_normals(3, 4, 2, [0.0, 0.1, -0.2], 0.0)
    assert n.shape == (3, 4, 2, 3) and np.array_equal(n[0, 0, 0], [0.0, 0.0, 1.0])
    assert np.allclose(n[1, 3, 1], [0.0, -np.sin(0.1), np.cos(0.1)]) and np.allclose(np.sum(n * n, axis=-1), 1.0, atol=1e-15, rtol=0)


# ---- the C-ABI without a GPU: every refusal comes before the first HIP call -----------------------------------------------------------

def _host(b, cone, **kw):
    with pytest.raises(_lib.BmpcError) as e:
        bb.solve_host(b, num_iters=1, cone=cone, **kw)
    assert e.value.code == _lib.BAD_ARG
    return str(e.value)


def test_batch_refusals():
    b = problems.make_batch("solo12_trot", 2, H=20)
    nrm = np.array(cone_frame_np.normals(2, 20, 4))
    with pytest.raises(ValueError):      # normals without "euclidean"
        bb.solve_host(b, cone=dict(projection="reference", normals=nrm))
    with pytest.raises(ValueError):
        bb.solve_host(b, cone=dict(normals=nrm))
    for shape in ((2, 20, 4), (2, 20, 3, 3), (3, 20, 4, 3), (2, 19, 4, 3), (20, 4, 3)):
        with pytest.raises(ValueError):
            bb.solve_host(b, cone=dict(EUCLID, normals=np.zeros(shape)))
    assert "fp64" in _host(b, dict(EUCLID, normals=nrm), precision="f32")
    long = problems.make_batch("solo12_trot", 2, H=64)
    assert "64 knots" in _host(long, dict(EUCLID, normals=np.array(cone_frame_np.normals(2, 64, 4))))
    for bad in ((0.0, 0.0, 1.0 + 1e-8), (0.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (0.0, np.inf, 1.0), (0.6, 0.0, 0.8 + 1e-8)):
        n = nrm.copy()
        n[1, 7, 2] = bad
        assert "unit length" in _host(b, dict(EUCLID, normals=n))
    n = nrm[:1].copy()      # ... in a shared set too
    n[0, 19, 3] = (0.0, 0.0, 0.99)
    assert "unit length" in _host(b, dict(EUCLID, normals=n))
    raw = cone_np.raw_batch(b)
    with pytest.raises(ValueError):
        bb.solve_host(b, raw=dict(raw, Qf_off=np.zeros((1, 19, 12))), cone=dict(EUCLID, normals=nrm))
    # straight to the C calls: normals under projection 0, strides, n_eff
    lib = _lib.lib()
    d = _lib.Batch()
    lib.bmpc_batch_defaults(C.byref(d))
    d.B, d.n_col, d.n_eff = 2, 20, 4
    flat = np.ascontiguousarray(nrm)
    calls = (lambda c, f: lib.bmpc_biconvex_solve_batch_cone_frames_host(C.byref(d), c, f),
             lambda c, f: lib.bmpc_biconvex_solve_batch_cone_frames_device(C.byref(d), c, f, None))
    one = _lib.Cone(projection=1)
    for fn in calls:
        for cone in (None, C.byref(_lib.Cone(projection=0))):
            assert fn(cone, C.byref(_lib.ContactFrame(normals=flat.ctypes.data, snormals=240))) == _lib.BAD_ARG and "projection = 1" in _lib.last_error()
        for stride in (-1, 239, (1 << 26) + 1):
            assert fn(C.byref(one), C.byref(_lib.ContactFrame(normals=flat.ctypes.data, snormals=stride))) == _lib.BAD_ARG
            assert "snormals" in _lib.last_error() and "2^26" in _lib.last_error()
        assert fn(C.byref(_lib.Cone(projection=2)), C.byref(_lib.ContactFrame(normals=flat.ctypes.data, snormals=240))) == _lib.BAD_ARG and "projection must be" in _lib.last_error()
    d.n_eff = 3
    for fn in calls:
        assert fn(C.byref(one), C.byref(_lib.ContactFrame(normals=flat.ctypes.data, snormals=0))) == _lib.BAD_ARG and "n_eff" in _lib.last_error()
    d.n_eff, d.precision = 4, 1
    for fn in calls:
        assert fn(C.byref(one), C.byref(_lib.ContactFrame(normals=flat.ctypes.data, snormals=0))) == _lib.BAD_ARG and "fp64" in _lib.last_error()
    d.precision, d.n_col = 0, 64
    for fn in calls:
        assert fn(C.byref(one), C.byref(_lib.ContactFrame(normals=flat.ctypes.data, snormals=0))) == _lib.BAD_ARG and "64 knots" in _lib.last_error()


def _handle(b, H):
    mp = BiconvexMP(b.m, H, b.E)
    for t in range(H):
        mp.set_contact_plan(b.cnt_plan[0, t], b.dt[0, t])
    return mp


def _refused(mp, b, word):
    with pytest.raises(_lib.BmpcError) as e:
        mp.optimize(b.x_init[0], 1)
    assert e.value.code == _lib.BAD_ARG and word in str(e.value), str(e.value)


def test_handle_refusals():
    b = problems.make_batch("solo12_trot", 1, H=20)
    mp = _handle(b, 20)
    nrm = np.array(cone_frame_np.normals(1, 20, 4)[0])
    for shape in ((20, 4), (4,), (19, 4, 3), (20, 4, 4)):
        with pytest.raises(ValueError):
            mp.set_contact_normals(np.zeros(shape))
    for bad in ((0.0, 0.0, 1.0 + 1e-8), (np.nan, 0.0, 1.0), (0.0, 0.0, np.inf), (0.0, 0.0, 0.0)):
        n = nrm.copy()
        n[3, 1] = bad
        with pytest.raises(_lib.BmpcError) as e:
            mp.set_contact_normals(n)
        assert e.value.code == _lib.BAD_ARG and "unit length" in str(e.value)
    # normals under the reference's projection
    mp.set_contact_normals(nrm)
    _refused(mp, b, "set_cone_projection")
    mp.set_contact_normals(None)      # (back to world z: nothing to refuse before the launch -- not tried here, it needs a GPU)
    mp.set_contact_normals(nrm[0])    # one normal per foot
    _refused(mp, b, "set_cone_projection")
    # block and band costs
    mp.set_cone_projection("euclidean")
    r = cone_np.raw_of(b, 0)
    blk = np.diag(r["Qf"])
    blk[0, 1] = blk[1, 0] = 1e-5
    mp.set_cost_f(blk, np.zeros(mp.nf))
    _refused(mp, b, "diagonal costs only")
    band = np.diag(r["Qx"]) + np.diag(np.full(mp.nx - 9, 0.5), 9) + np.diag(np.full(mp.nx - 9, 0.5), -9)
    mp.set_cost_f(r["Qf"], np.zeros(mp.nf))
    mp.set_cost_x(band, r["qx"])
    _refused(mp, b, "diagonal costs only")
    # more than 64 knots
    big = problems.make_batch("solo12_trot", 1, H=64)
    mp = _handle(big, 64)
    mp.set_cone_projection("euclidean")
    mp.set_contact_normals(np.array([0.0, 0.0, 1.0]) * np.ones((4, 1)))
    _refused(mp, big, "64 knots")


def test_rotation_matrices_as_contact_frames_refusals():
    b = problems.make_batch("biped_walk", 1, H=3)
    mp = _handle(b, 3)
    R = _rotations(6, 5)
    for i in range(5):      # too few
        mp.set_rotation_matrix_f(R[i])
    with pytest.raises(_lib.BmpcError) as e:
        mp.use_rotation_matrices_as_contact_frames()
    assert e.value.code == _lib.BAD_ARG and "n_col * n_eff = 6" in str(e.value) and "holds 5" in str(e.value)
    mp.set_rotation_matrix_f(R[5])
    mp.use_rotation_matrices_as_contact_frames()      # exactly n_col * n_eff
    mp.set_rotation_matrix_f(R[0])                    # too many
    with pytest.raises(_lib.BmpcError) as e:
        mp.use_rotation_matrices_as_contact_frames()
    assert e.value.code == _lib.BAD_ARG and "holds 7" in str(e.value)
    mp = _handle(b, 3)
    for i in range(6):      # a third row that is no unit vector
        mp.set_rotation_matrix_f(R[i] * (1.001 if i == 4 else 1.0))
    with pytest.raises(_lib.BmpcError) as e:
        mp.use_rotation_matrices_as_contact_frames()
    assert e.value.code == _lib.BAD_ARG and "third row" in str(e.value) and "normal 4" in str(e.value)


def test_dropin_exposes_the_setters():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dropin_biconvex_mpc_cpp", os.path.join(ROOT, "bunmpc_amd", "dropin", "biconvex_mpc_cpp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in ("set_contact_normals", "use_rotation_matrices_as_contact_frames", "set_cone_projection", "set_friction_coefficients"):
        assert callable(getattr(mod.BiconvexMP, name))


_I, _P = C.c_int, C.c_void_p
_NEW = {"bmpc_contact_frame_struct_size": (_I, []),
        "bmpc_biconvex_solve_batch_cone_frames_device": (_I, [_P, _P, _P, _P]),
        "bmpc_biconvex_solve_batch_cone_frames_host": (_I, [_P, _P, _P]),
        "bmpc_biconvex_set_contact_normals": (_I, [_P, _P]),
        "bmpc_biconvex_set_contact_normals_from_rotations": (_I, [_P]),
        "bmpc_biconvex_cone_frame_kernel_scratch_bytes": (_I, [_I])}


def test_bindings_match_the_header(hiplib):
    """the new entry points' signatures as the binding reads them from include/bunmpc.h (tests/test_abi_cpu.py holds the whole
    table); the structs' sizes"""
    for name, sig in _NEW.items():
        assert _lib._SIGS[name] == sig, name
    assert hiplib.bmpc_contact_frame_struct_size() == C.sizeof(_lib.ContactFrame) == 16
    assert hiplib.bmpc_cone_struct_size() == C.sizeof(_lib.Cone) == 24
    assert hiplib.bmpc_biconvex_cone_frame_kernel_scratch_bytes(3) == -1
