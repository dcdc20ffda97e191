"""CPU side of the per-pass checks of the IK-DDP kernels (the GPU side is tests/test_ik_passes_gpu.py): the references and the
case set of tests/ik_passes_np.py are themselves pinned here --
  a. the two CPU twins agree on every case (their gap per quantity is the yardstick the kernels are held to);
  b. unpack_node inverts an independently written packer of the compact hand-over format;
  c. the stand-alone Riccati reference reproduces the gains of the numpy twin's SolverDDP;
  d. each of eleven single-term mutations of a reference is flagged by the GPU test's own comparison at >= 100 x its tolerance
     on at least one case: neither the tolerances nor the inputs are too mild to see a wrong term."""
import functools

import numpy as np
import pytest

from oracle import ik_ddp_np, rbd_np as rb
from tests import ik_passes_np as P

NV, NDX = P.NV, P.NDX


@functools.lru_cache(maxsize=None)
def case_set():
    return {c.name: c for c in P.cases("all")}


@functools.lru_cache(maxsize=None)
def twins(name):
    return P.twins_on_case(case_set()[name])


SMALL = [c.name for c in P.cases("small")]
ALL = list(case_set())


# ---------------------------------------------------------------------------------------- a ---
@pytest.mark.parametrize("name", ALL)
def test_twins_agree_on_the_cases(name):
    """ik_ddp_np.node_calc(diff=True) against oracle/ik_oracle_c.node (and the two state differences for the gaps) on every case:
    a class where they differ by more than 1e-9 would be ill-conditioned or a twin bug.  Prints the gap per quantity."""
    tw = twins(name)
    print("twin gap %-40s %s" % (name, "  ".join("%s %.1e" % (q, tw["gap"][q]) for q in P.DERIV_QUANTITIES)))
    for q in P.DERIV_QUANTITIES:
        assert tw["gap"][q] < 1e-9, (name, q, tw["gap"][q])
        assert tw["tol"][q] == max(10 * tw["gap"][q], P.FLOOR[q])


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 1e-18


# ---------------------------------------------------------------------------------------- b ---
def pack_node(Lq, M, w, dv):
    """The compact form as calc_assemble stores it (ik_ddp.hip, the Lqq[...] / Hn[...] stores), written lane by lane as the kernel
    does -- independent of unpack_lxx's reshapes.  Lq: L_qq' (18 x 18), M (6 x 36), w = sc wm, dv: velocity diagonal (18)."""
    lqq, hn = np.full(P.LQQ, np.nan), np.full(P.HN, np.nan)
    for lane in range(64):
        li, lk = lane & 15, lane >> 4
        for v in range(4):
            lqq[v * 64 + lane] = Lq[lk + 4 * v, li]
            if li < 2:
                lqq[256 + (v * 4 + lk) * 2 + li] = Lq[lk + 4 * v, 16 + li]
        if li < 2 and lk < 2:
            lqq[288 + lk * 2 + li] = Lq[16 + lk, 16 + li]
        if lane < NDX:
            for k in range(6):
                hn[k * NDX + lane] = M[k, lane]
        if lane < 16:
            hn[P.HN_D11 + lane] = dv[lane - 2] if lane >= 2 else 0.0
        elif lane < 20:
            hn[P.HN_D22 + lane - 16] = dv[lane - 2]
        elif lane == 20:
            hn[P.HN_W] = w
    return lqq, hn


def twin_pieces(case, b, t):
    """what the compact form holds of node t, from the numpy twin's kinematics: L_qq', M, sc wm, the velocity diagonal"""
    d = twins(case.name)["np"][(b, t)]
    x = case.xs[b, t]
    kin = rb.Kin(case.model, x[:P.NQ], x[P.NQ:])
    M = np.hstack([kin.dh_dq(), kin.centroidal_map()])
    sc = 1.0 if t == case.T else case.dt[b, t]
    tk = case.tasks[b, t]
    w = sc * tk[24]
    dv = sc * tk[31] * case.node_weights(b, t)[0][NV:]
    Lq = d["Lxx"][:NV, :NV] - w * (M[:, :NV].T @ M[:, :NV])
    return Lq, M, w, dv


def test_unpack_node_round_trip():
    """exact on integer-valued pieces (every product and sum is exact in fp64, so the dense matrix assembled entry by entry must come
    back bit for bit); to rounding on the twin's own L_xx; F_x / F_u exact against the numpy twin's from the same Jintegrate blocks"""
    rng = np.random.default_rng(7)
    for _ in range(4):
        Lq = rng.integers(-50, 50, (NV, NV)).astype(float)
        Lq = Lq + Lq.T
        M = rng.integers(-9, 9, (6, NDX)).astype(float)
        w, dv = float(rng.integers(1, 9)), rng.integers(0, 99, NV).astype(float)
        want = np.zeros((NDX, NDX))
        for i in range(NDX):
            for j in range(NDX):
                want[i, j] = (Lq[i, j] if i < NV and j < NV else 0.0) + w * sum(M[k, i] * M[k, j] for k in range(6)) + (dv[i - NV] if i == j >= NV else 0.0)
        lqq, hn = pack_node(Lq, M, w, dv)
        assert np.array_equal(P.unpack_lxx(lqq, hn), want)
        assert not np.array_equal(P.unpack_lxx(lqq, hn, "tile01_transposed"), want)
    case = case_set()["solo12_T10_a0.5_node_vel10"]
    lay = P.layout(case.T)
    for b, t in ((0, 0), (1, 3), (2, case.T), (4, 7)):
        d = twins(case.name)["np"][(b, t)]
        lqq, hn = pack_node(*twin_pieces(case, b, t))
        ws = np.zeros(lay["total"])
        ws[lay["Lqq"] + t * P.LQQ: lay["Lqq"] + (t + 1) * P.LQQ] = lqq
        ws[lay["Hn"] + t * P.HN: lay["Hn"] + (t + 1) * P.HN] = hn
        ws[lay["Lx"] + t * NDX: lay["Lx"] + (t + 1) * NDX] = d["Lx"]
        if t < case.T:
            dt = case.dt[b, t]
            x, u = case.xs[b, t], case.us[b, t]
            J1, J2 = rb.state_jintegrate(case.model, x, np.concatenate([x[P.NQ:] * dt + u * dt * dt, u * dt]))
            ws[lay["A6"] + 36 * t: lay["A6"] + 36 * (t + 1)] = J1[:6, :6].reshape(-1)
            ws[lay["B6"] + 36 * t: lay["B6"] + 36 * (t + 1)] = J2[:6, :6].reshape(-1)
            ws[lay["Lu"] + t * NV: lay["Lu"] + (t + 1) * NV] = d["Lu"]
            ws[lay["Luu"] + t * NV: lay["Luu"] + (t + 1) * NV] = d["Luu"]
            ws[lay["xnext"] + t * P.NX: lay["xnext"] + (t + 1) * P.NX] = d["xnext"]
        got = P.unpack_node(ws, lay, t, case.dt[b, min(t, case.T - 1)], case.T)
        assert np.abs(got["Lxx"] - d["Lxx"]).max() <= 4 * P.EPS * np.abs(d["Lxx"]).max()       # (a - w m m) + w m m: two roundings at the size of the entry
        assert np.array_equal(got["Lx"], d["Lx"])
        if t < case.T:
            for q in ("Fx", "Fu", "Lu", "Luu", "xnext"):
                assert np.array_equal(got[q], d[q]), q


# ---------------------------------------------------------------------------------------- c ---
@pytest.mark.parametrize("name", ["go2_T7_a1e-4_node_xreg1", "solo12_T10_a0.5_node_vel10", "solo12_T10_indefinite"])
def test_riccati_reference_reproduces_the_numpy_ddp(name):
    """solve_ddp(maxiter = 1) runs one backward pass from its cold start (neutral states, zero controls, gaps): riccati(float64) on
    the derivatives of that trajectory must give its gains.  Both are backward-stable fp64 eliminations of the same matrices (LAPACK
    there, written out here), so they sit within a small multiple of each other's distance to the long-double result."""
    case = case_set()[name]
    model, T = case.model, case.T
    for b in (0, 3):
        prob = case.np_problem(b)
        r = ik_ddp_np.solve_ddp(prob, case.x0[b], maxiter=1)
        zero = np.concatenate([rb.neutral(model), np.zeros(NV)])
        data = [ik_ddp_np.node_calc(prob, t, zero, np.zeros(NV) if t < T else None, diff=True) for t in range(T + 1)]
        fs = [rb.state_diff(model, zero, case.x0[b])] + [rb.state_diff(model, zero, data[t]["xnext"]) for t in range(T)]
        ref, f64, bound = P.riccati_bounds(data, fs, 1e-9, False)
        assert f64["retries"] == ref["retries"] and not ref["gave_up"]
        if case.indefinite:
            assert ref["retries"] >= 3          # the pass did fail and start again
        err = P.riccati_errors(dict(K=np.array(r["K"]), k=np.array(r["k"]), d1=ref["d1"], d2=ref["d2"], stop=ref["stop"]), ref)
        print("%s problem %d: retries %d, solve_ddp vs long double K %.1e k %.1e; float64 bound K %.1e k %.1e"
              % (name, b, ref["retries"], err["K"], err["k"], bound["K"], bound["k"]))
        for q in ("K", "k"):
            assert err[q] <= 10 * bound[q] + 64 * P.EPS, (q, err[q], bound[q])


# ---------------------------------------------------------------------------------------- d ---
def _ratio(mut, ref, tol, quantities):
    return max(P.node_error(mut, ref, q) / tol[q] for q in quantities if q in ref)


def _twin_mutation_ratio(case, kind):
    """largest (error of the mutated numpy twin against the true one) / (the case's tolerance) over a case's sampled nodes"""
    tw = twins(case.name)
    worst = 0.0
    tasks = case.tasks
    if kind == "slot_weights_swapped":
        tasks = case.tasks.copy()
        tasks[:, :, [0, 5]] = case.tasks[:, :, [5, 0]]
    probs = {}
    for b, t in case.np_nodes():
        if b not in probs:
            probs[b] = case.np_problem(b, tasks)
        ref = tw["np"][(b, t)]
        if kind in ("jlog6_identity", "frame_jacobian_at_parent", "momentum_without_dh_dq"):
            with P.mutated_twin(kind):
                mut = P.np_twin_node(probs[b], case, b, t)
        elif kind == "slot_weights_swapped":
            mut = P.np_twin_node(probs[b], case, b, t)
        elif kind == "dt_dropped_from_B" and t < case.T:
            mut = dict(ref, Fx=ref["Fx"].copy())
            mut["Fx"][:NV, NV:] /= case.dt[b, t]
        elif kind == "Luu_without_sc" and t < case.T:
            mut = dict(ref, Luu=ref["Luu"] / case.dt[b, t])
        elif kind in ("tile01_transposed", "no_velocity_diagonal"):
            lqq, hn = pack_node(*twin_pieces(case, b, t))
            mut = dict(ref, Lxx=P.unpack_lxx(lqq, hn, kind))
        else:
            continue
        worst = max(worst, _ratio(mut, ref, tw["tol"], ("cost", "xnext", "Fx", "Fu", "Lx", "Lxx", "Lu", "Luu")))
    return worst


def _riccati_mutation_ratio(case, kind):
    """largest (error of the mutated float64 Riccati pass against the long-double one) / (bound of that problem) over a case"""
    tw = twins(case.name)
    worst = 0.0
    rng = np.random.default_rng(11)
    for b in range(case.B):
        data = [dict(d) for d in tw["c"][b]]
        for t in range(case.T):
            data[t]["Fx"], data[t]["Fu"] = tw["c"][b][t]["Fx"], tw["c"][b][t]["Fu"]
        if kind == "no_symmetrise":
            # Q_xx - Q_xu K is symmetric whenever L_xx is: dropping the symmetrisation shows only on an L_xx that is not.  The
            # kernels cannot be handed one (their tile (0,0) is symmetric to rounding); this input exists for this mutation alone.
            for d in data:
                E = rng.standard_normal((NDX, NDX))
                d["Lxx"] = d["Lxx"] + 1e-6 * np.abs(d["Lxx"]).max() * (E - E.T)
        fs = tw["fs_c"][b]
        ref, f64, bound = P.riccati_bounds(data, fs, case.xreg, case.feasible)
        mut = P.riccati(data, fs, case.xreg, case.feasible, np.float64, mut=kind)
        if bound is None or mut["gave_up"]:
            continue
        if mut["retries"] != ref["retries"]:
            return np.inf
        err = P.riccati_errors(mut, ref)
        worst = max(worst, max(err[q] / bound[q] for q in P.RICCATI_QUANTITIES if bound[q] > 0))
    return worst


MUTATIONS = [   # (name in the issue's order, kind, where it is applied, cases that should show it)
    ("1 Jlog6 block replaced by the identity", "jlog6_identity", "twin", ["solo12_T7_a3.0_problem", "solo12_T10_a0.5_node_vel10"]),
    ("2 dt dropped from the B block of F_x", "dt_dropped_from_B", "twin", ["solo12_T1_a0_shared"]),
    ("3 two frame-slot weights swapped", "slot_weights_swapped", "twin", ["go2_T7_a1e-4_node_xreg1"]),
    ("4 one frame Jacobian taken at the parent body", "frame_jacobian_at_parent", "twin", ["go2_T7_a1e-4_node_xreg1"]),
    ("5 M without its dh/dq half", "momentum_without_dh_dq", "twin", ["solo12_T10_a0.5_node_vel10"]),
    ("6 tile (0,1) transposed in unpacking", "tile01_transposed", "twin", ["solo12_T2_a1e-9_problem_feas_xreg1"]),
    ("7 V_xx not symmetrised", "no_symmetrise", "riccati", ["go2_T7_a1e-4_node_xreg1"]),
    ("8 xreg not added to V_xx", "no_xreg", "riccati", ["go2_T7_a1e-4_node_xreg1", "go2_T2_a3.0_shared_xreg1"]),
    ("9 gap term V_xx fs dropped", "no_gap_term", "riccati", ["solo12_T7_a3.0_problem"]),
    ("10 d11 / d22 (velocity diagonal) dropped", "no_velocity_diagonal", "twin", ["solo12_T2_a1e-9_problem_feas_xreg1"]),
    ("11 L_uu without sc", "Luu_without_sc", "twin", ["solo12_T1_a0_shared"]),
]


@pytest.mark.parametrize("label,kind,where,names", MUTATIONS, ids=[m[1] for m in MUTATIONS])
def test_the_comparison_sees_a_single_wrong_term(label, kind, where, names):
    f = _twin_mutation_ratio if where == "twin" else _riccati_mutation_ratio
    ratios = {n: f(case_set()[n], kind) for n in names}
    print("mutation %-48s error / tolerance: %s" % (label, "  ".join("%s %.1e" % kv for kv in ratios.items())))
    assert max(ratios.values()) >= 100.0, (label, ratios)
