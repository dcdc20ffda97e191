"""The CPU twin of the Euclidean friction-cone projection about per-contact surface normals (bmpc_contact_frame_t) and the shared pieces
of its tests: the projection, the normals of the cases, and the numpy restatement of the solve with it -- tests/cone_np.py's cases and
restatement with this projection as its argument."""
import functools

import numpy as np

from tests import cone_np

MAX_TILT_DEG = 25.0


def project_frame(v, mu, normals, count=None):
    """Nearest point of the cone |f - (n.f) n| <= mu n.f for every 3-vector of v (any shape whose size is a multiple of 3), mu a scalar or
    one coefficient per vector, normals one unit vector per vector of v (or one for all).  With fn = n.f, ft = f - fn n, s2 = |ft|^2:
    the origin in the polar cone (fn <= 0, mu^2 s2 <= fn^2; wins at the origin), f itself -- its bits -- inside (fn >= 0,
    s2 <= mu^2 fn^2), otherwise k ft + t n with t = (mu s + fn) / (mu^2 + 1), k = mu t / s.  The sums are taken in the kernel's order
    (fn = nx fx + (ny fy + nz fz), s2 = ftx^2 + (ftz^2 + fty^2)): with n = (0, 0, 1) every extra term is an exact zero and the values
    are cone_np.project's.  count: a list of three ints, increased by the vectors on the zero / inside / surface branch."""
    y = np.array(v, dtype=np.float64).reshape(-1, 3)
    n = np.broadcast_to(np.asarray(normals, dtype=np.float64).reshape(-1, 3), y.shape)
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64).reshape(-1), (y.shape[0],))
    fn = n[:, 0] * y[:, 0] + (n[:, 1] * y[:, 1] + n[:, 2] * y[:, 2])
    ft = y - fn[:, None] * n
    s2 = ft[:, 0] * ft[:, 0] + (ft[:, 2] * ft[:, 2] + ft[:, 1] * ft[:, 1])
    mu2 = mu * mu
    zero = (fn <= 0) & (mu2 * s2 <= fn * fn)
    inside = ~zero & (fn >= 0) & (s2 <= mu2 * (fn * fn))
    surf = ~zero & ~inside
    out = y.copy()
    out[zero] = 0.0
    s = np.sqrt(s2[surf])
    t = (mu[surf] * s + fn[surf]) / (mu2[surf] + 1.0)
    k = mu[surf] * t / s
    out[surf] = t[:, None] * n[surf] + k[:, None] * ft[surf]
    if count is not None:
        count[0] += int(zero.sum()); count[1] += int(inside.sum()); count[2] += int(surf.sum())
    return out.reshape(np.shape(v))


def tilted(tilt, azimuth):
    """unit vectors at angle `tilt` from world z towards `azimuth` (radians; arrays of one shape): shape + (3,)"""
    return np.stack([np.sin(tilt) * np.cos(azimuth), np.sin(tilt) * np.sin(azimuth), np.cos(tilt)], axis=-1)


@functools.lru_cache(maxsize=None)
def normals(B, H, E):
    """(B, H, E, 3) unit normals, fixed seed per (H, E): tilt uniform in [0, 25] degrees about world z, azimuth uniform, per problem, knot
    and foot (shared: do not modify)"""
    rng = np.random.default_rng([20251018, H, E])
    tilt = np.deg2rad(rng.uniform(0.0, MAX_TILT_DEG, size=(B, H, E)))
    az = rng.uniform(0.0, 2.0 * np.pi, size=(B, H, E))
    return tilted(tilt, az)


def restatement(b, i, iters, mu, nrm, **kw):
    """cone_np.restatement of problem i with the projection about the normals nrm (H, E, 3); "branches" as there"""
    return cone_np.restatement(b, i, iters, mu, projection=lambda v, m, count: project_frame(v, m, nrm, count), **kw)


@functools.lru_cache(maxsize=None)
def twin(config, H, perturbed=False, with_qf=False):
    """the restatement of every problem of cone_np.case(config, H) with normals(6, H, E), computed once per process (shared: do not
    modify); perturbed: x_init[0] of every problem moved by one ulp"""
    b, mu, warm, iters = cone_np.case(config, H)
    nrm = normals(b.B, H, b.E)
    qf = cone_np.linear_force_cost(b) if with_qf else None
    return [restatement(b, i, iters, mu[i], nrm[i], warm=warm, L_f=cone_np.L_F, x_init=cone_np.one_ulp(b.x_init[i]) if perturbed else None,
                        qf=None if qf is None else qf[i]) for i in range(b.B)]


def cone_excess(F, mu, nrm):
    """(fn, |ft| - mu fn) of forces F against the cones about nrm: arrays of mu's shape"""
    F = np.asarray(F).reshape(np.shape(nrm))
    fn = np.sum(F * nrm, axis=-1)
    ft = F - fn[..., None] * nrm
    return fn, np.linalg.norm(ft, axis=-1) - mu * fn
