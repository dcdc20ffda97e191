"""Synthetic MPC problem batches at the centroidal level.

Host-side numpy restatement of the *inputs* the reference's Python harness hands to
`BiconvexMP` (contact plan, dt, X_nom, X_ter, bounds, weights), vectorised over the
batch axis.  Follows, without importing it,
  iterative_supervised_learning/examples/mpc/abstract_cyclic_gen.py:159-414  (create_cnt_plan)
  iterative_supervised_learning/examples/mpc/abstract_cyclic_gen.py:532-614  (create_costs)
  iterative_supervised_learning/examples/motions/cyclic/solo12_{trot,bound,jump}.py (gait constants)
at the centroidal level: the robot state enters only through CoM / foot positions
(no pinocchio), exactly as SURVEY.md 8d defines configs 1-4.  Go2 and "pace" do not
exist in the reference: those sets are synthetic (documented in DESIGN.md), as is the biped
(BIPED, BIPED_GAITS, make_batch("biped_walk")): two feet, n_eff = 2.
"""
from dataclasses import dataclass, field, replace

import numpy as np

GRAVITY = 9.81
FOOT_SIZE = 0.018          # abstract_cyclic_gen.py:31
BOUNDS_TILE = np.array([-0.45, -0.45, 0.0, 0.45, 0.45, 0.45])  # :92-97,611
BASE_SEED = 20250202


@dataclass
class GaitParams:
    """BiconvexMotionParams subset needed by the centroidal solve (weight_abstract.py:7-42)."""
    name: str
    gait_period: float
    stance_percent: tuple
    phase_offset: tuple
    gait_horizon: float
    W_X: np.ndarray
    W_X_ter: np.ndarray
    W_F: np.ndarray            # (3E,) one knot: E feet x 3
    nom_ht: float
    rho: float = 5e4
    gait_dt: float = 0.05
    step_ht: float = 0.075
    ori_correction: tuple = (0.3, 0.5, 0.4)

    @property
    def horizon(self):
        # abstract_cyclic_gen.py:125
        return int(np.round(self.gait_horizon * self.gait_period / self.gait_dt, 2))


@dataclass
class RobotParams:
    name: str
    mass: float
    feet_xy: np.ndarray        # (E,2) nominal foot xy (FL,FR,HL,HR; a biped: L,R)
    offsets_xy: np.ndarray     # (E,2) hip-minus-com offsets after rounding and +-0.04 widening
    com_height: float


# solo12.urdf link masses summed; feet under the hips
SOLO12 = RobotParams(
    "solo12", 2.50000279,
    np.array([[0.1946, 0.14695], [0.1946, -0.14695], [-0.1946, 0.14695], [-0.1946, -0.14695]]),
    np.array([[0.195, 0.142], [0.195, -0.142], [-0.195, 0.142], [-0.195, -0.142]]),
    0.23)
# synthetic Go2 (const.xacro masses/geometry)
GO2 = RobotParams(
    "go2", 15.097,
    np.array([[0.1934, 0.142], [0.1934, -0.142], [-0.1934, 0.142], [-0.1934, -0.142]]),
    np.array([[0.193, 0.182], [0.193, -0.182], [-0.193, 0.182], [-0.193, -0.182]]),
    0.30)

# motions/cyclic/solo12_trot.py:16-41
TROT = GaitParams(
    "trot", 0.5, (0.6,) * 4, (0.0, 0.5, 0.5, 0.0), 2.0,
    np.array([1e-5, 1e-5, 1e5, 1e1, 1e1, 2e2, 1e4, 1e4, 1e4]),
    10 * np.array([1e5, 1e-5, 1e5, 1e1, 1e1, 2e2, 1e5, 1e5, 1e5]),
    np.array(4 * [1e1, 1e1, 1e1]), 0.2, step_ht=0.075, ori_correction=(0.3, 0.5, 0.4))
# motions/cyclic/solo12_trot.py:46-74 (trot_turn): the second pair 0.4 of a period behind, one period of horizon (H = 10, H_ik = 5), no
# roll correction; dataset.GAIT_VALUE has no entry for its name, so its gait value in vc_goals is that of an unknown gait
TROT_TURN = GaitParams(
    "trot_turn", 0.5, (0.6,) * 4, (0.0, 0.4, 0.4, 0.0), 1.0,
    TROT.W_X.copy(), TROT.W_X_ter.copy(), TROT.W_F.copy(), 0.2, step_ht=0.05, ori_correction=(0.0, 0.5, 0.4))
# motions/cyclic/solo12_bound.py:16-44
BOUND = GaitParams(
    "bound", 0.3, (0.5,) * 4, (0.0, 0.0, 0.5, 0.5), 4.0,
    np.array([1e-5, 1e-5, 5e4, 1e1, 1e1, 1e3, 5e3, 1e4, 5e3]),
    10 * np.array([1e-5, 1e-5, 5e4, 1e1, 1e1, 1e3, 1e4, 1e4, 1e4]),
    np.array(4 * [1e1, 1e1, 1.5e1]), 0.25, step_ht=0.07, ori_correction=(0.2, 0.8, 0.8))
# motions/cyclic/solo12_jump.py:17-43
JUMP = GaitParams(
    "jump", 0.5, (0.3,) * 4, (0.7, 0.7, 0.7, 0.7), 3.0,
    TROT.W_X.copy(), TROT.W_X_ter.copy(), np.array(4 * [1e1, 1e1, 1.5e1]), 0.25,
    step_ht=0.05, ori_correction=(0.2, 0.5, 0.4))
# synthetic: trot weights, lateral pairs in phase
PACE = GaitParams(
    "pace", 0.5, (0.6,) * 4, (0.0, 0.5, 0.0, 0.5), 2.0,
    TROT.W_X.copy(), TROT.W_X_ter.copy(), TROT.W_F.copy(), 0.2)
GAITS = {"trot": TROT, "bound": BOUND, "jump": JUMP, "pace": PACE}

# synthetic biped, Bolt-sized (the reference's IK examples target bipeds; its centroidal demo runs n_eff = 2): 1.3 kg, CoM at
# 0.30 m, feet (L, R) 0.08 m either side of the CoM, hips above them.  Not a robot description: numbers of the right size only.
BIPED = RobotParams(
    "biped", 1.3,
    np.array([[0.0, 0.08], [0.0, -0.08]]),
    np.array([[0.0, 0.08], [0.0, -0.08]]),
    0.30)
# biped gaits, trot's state weights and timing (0.05 s knots, 20 per plan), forces 2 feet x 3:
#   walk   each foot 60 % on the ground, half a period apart: two double-support phases per period
#   stand  both feet always on the ground
#   hop    both feet together, 60 % stance, then a flight phase of 0.2 s
BIPED_WALK = GaitParams(
    "biped_walk", 0.5, (0.6, 0.6), (0.0, 0.5), 2.0,
    TROT.W_X.copy(), TROT.W_X_ter.copy(), np.array(2 * [1e1, 1e1, 1e1]), 0.30, step_ht=0.05)
BIPED_STAND = GaitParams(
    "biped_stand", 0.5, (1.0, 1.0), (0.0, 0.0), 2.0,
    TROT.W_X.copy(), TROT.W_X_ter.copy(), np.array(2 * [1e1, 1e1, 1e1]), 0.30, step_ht=0.0)
BIPED_HOP = GaitParams(
    "biped_hop", 0.5, (0.6, 0.6), (0.0, 0.0), 2.0,
    TROT.W_X.copy(), TROT.W_X_ter.copy(), np.array(2 * [1e1, 1e1, 1.5e1]), 0.30, step_ht=0.05)
BIPED_GAITS = {"walk": BIPED_WALK, "stand": BIPED_STAND, "hop": BIPED_HOP}
# friction coefficient of the biped batches: 10, as for the synthetic Go2.  With the reference's mu = 1 the CPU oracle solves the
# biped_walk problems without NaN, but its squared-norm "SoC" projection (fista.cpp:52-70) inflates the forces of long solves: at 100
# ADMM iterations up to 174 N on a 1.3 kg robot, against 24 N with mu = 5 or 10 (256 problems; ten iterations: the same 15 N for all).
BIPED_MU = 10.0


# ---------------------------------------------------------------- gait phase ---
def gait_phi(t, period, offset):
    """gait_planner.cpp:41-44 (vectorised)."""
    return np.fmod(t + offset * period, period)


def gait_phase(t, period, stance_percent, offset):
    """gait_planner.cpp:46-58, scalar overload incl. the 1e-4 slack."""
    st = period * stance_percent
    phi = gait_phi(t, period, offset)
    return ((phi <= st) | (np.abs(phi - st) < 1e-4)).astype(np.float64)


def gait_percent_in_phase(t, period, stance_percent, offset):
    """gait_planner.cpp:112-128."""
    st = period * stance_percent
    phi = gait_phi(t, period, offset)
    with np.errstate(divide="ignore", invalid="ignore"):     # 100 % stance: the swing branch is never selected
        return np.where(phi <= st, phi / st, (phi - st) / (period - st))


# ------------------------------------------------------------- contact plan ---
def _terrain_call(fn, x, y, problem):
    """fn = height_map.getHeight / getNormal at the points (x, y) (arrays of one shape): a terrain.HeightMap takes the arrays (and,
    with one terrain per problem, the points' problem indices); any other object is called point by point with scalars, as the
    reference calls it"""
    from .terrain import HeightMap
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if isinstance(getattr(fn, "__self__", None), HeightMap):
        return fn(x, y, problem=problem) if fn.__self__.per_problem else fn(x, y)
    vals = [np.asarray(fn(float(a), float(b)), dtype=np.float64) for a, b in zip(x.reshape(-1), y.reshape(-1))]
    return np.array(vals).reshape(x.shape + vals[0].shape) if vals else np.zeros(x.shape)


def _problem_index(problem, shape):
    """the problem index of every point of an array whose leading axis runs over the problems `problem` (None: 0 .. B - 1)"""
    p = np.arange(shape[0]) if problem is None else np.asarray(problem, dtype=np.int64)
    return np.broadcast_to(p.reshape((shape[0],) + (1,) * (len(shape) - 1)), shape)


def terrain_normals(cnt_plan, height_map, problem=None):
    """normals (B, H, E, 3): height_map.getNormal at every knot's (x, y) of cnt_plan (B, H, E, 4) -- what solve_host / DeviceBatch
    take as cone=dict(projection="euclidean", normals=...).  problem (B,): the terrain of each row under a per-problem HeightMap
    (default: row b has terrain b)."""
    x, y = cnt_plan[..., 1], cnt_plan[..., 2]
    return np.ascontiguousarray(_terrain_call(height_map.getNormal, x, y, _problem_index(problem, x.shape)))


def contact_plan(gait, robot, H, t0, com_xy, z_height, feet0, v_des, w_des, hip_offsets=None, height_map=None, problem=None):
    """create_cnt_plan (abstract_cyclic_gen.py:159-414), data path (no MCTS / noise), vectorised over the batch.
      t0 (B,), com_xy (B,2) already rounded, z_height (B,), feet0 (B,4,3) already rounded,
      v_des (B,3) in the yaw frame (yaw = 0 here, R = I), w_des (B,)
    E feet, as many as the gait has (4 for the quadrupeds, 2 for the biped; feet0 (B,E,3))
    height_map: an object with getHeight(x, y) (terrain.HeightMap, or the reference's duck type): a new stance location and every
    swing location get z = getHeight(x, y) + FOOT_SIZE (:333-337, :370-374); knot 0 stays the current feet and a continuing stance
    copies the previous knot.  problem (B,): with one terrain per problem, the terrain of each row (default: row b has terrain b).
    returns cnt_plan (B,H,E,4), swing_time (B,H,E), dt (B,H)."""
    B = t0.shape[0]
    E = len(gait.stance_percent)
    gdt = gait.gait_dt
    cnt = np.zeros((B, H, E, 4))
    swing = np.zeros((B, H, E))
    vtrack = v_des[:, 0:2]
    # np.cross(ang_step(2-vector), [0,0,w]) -> (a_y w, -a_x w, 0)   (:285-286)
    ang2 = 0.5 * np.sqrt(z_height / GRAVITY)[:, None] * vtrack
    ang_step = np.stack([ang2[:, 1] * w_des, -ang2[:, 0] * w_des], axis=1)
    for i in range(H):
        for j in range(E):
            sp, off = gait.stance_percent[j], gait.phase_offset[j]
            if i == 0:
                ph = gait_phase(t0, gait.gait_period, sp, off)
                cnt[:, 0, j, 0] = ph
                cnt[:, 0, j, 1:4] = feet0[:, j]
                continue
            ft = np.round(t0 + i * gdt, 3)
            ph = gait_phase(ft, gait.gait_period, sp, off)
            hoff = robot.offsets_xy[j][None, :] if hip_offsets is None else hip_offsets[:, j]   # (R_yaw offsets[j])[0:2]
            hip_loc = com_xy + hoff + i * gdt * vtrack
            raibert = 0.5 * vtrack * gait.gait_period * sp - 0.05 * (vtrack - v_des[:, 0:2])
            per_ph = np.round(gait_percent_in_phase(ft, gait.gait_period, sp, off), 3)
            prev_on = cnt[:, i - 1, j, 0] == 1
            # stance, continuing contact: copy; stance, new contact: raibert + hip + ang
            new_xy = raibert + hip_loc + ang_step
            sw_xy = np.where((per_ph < 0.5)[:, None], hip_loc + ang_step,
                             hip_loc + ang_step + raibert)
            on = ph == 1
            xy = np.where(on[:, None], np.where(prev_on[:, None], cnt[:, i - 1, j, 1:3], new_xy),
                          sw_xy)
            ground = FOOT_SIZE if height_map is None else \
                _terrain_call(height_map.getHeight, xy[:, 0], xy[:, 1], _problem_index(problem, (B,))) + FOOT_SIZE
            z = np.where(on & prev_on, cnt[:, i - 1, j, 3], ground)
            cnt[:, i, j, 0] = ph
            cnt[:, i, j, 1:3] = xy
            cnt[:, i, j, 3] = z
            swing[:, i, j] = np.where(~on & (per_ph - 0.5 < 0.02), 1.0, 0.0)
    dt = np.full((B, H), gdt)
    dt0 = gdt - np.round(np.remainder(t0, gdt), 2)   # :385-388
    dt[:, 0] = np.where(dt0 == 0, gdt, dt0)
    return cnt, swing, dt


def centroidal_costs(gait, H, x_init, v_des, dt, amom=None):
    """create_costs, dynamics part (abstract_cyclic_gen.py:564-607), w_des = 0 branch unless
    yaw momentum is supplied through amom.  Returns X_nom (B,9H), X_ter (B,9)."""
    B = x_init.shape[0]
    if amom is None:
        amom = np.zeros((B, 3))
    X_nom = np.zeros((B, H, 9))
    X_nom[:, :, 0] = x_init[:, 0:1]
    for i in range(1, H):
        X_nom[:, i, 0] = X_nom[:, i - 1, 0] + v_des[:, 0] * dt[:, i]
        X_nom[:, i, 1] = X_nom[:, i - 1, 1] + v_des[:, 1] * dt[:, i]
    X_nom[:, :, 2] = gait.nom_ht
    X_nom[:, :, 3:6] = v_des[:, None, :]
    X_nom[:, :, 6:9] = (amom * np.asarray(gait.ori_correction))[:, None, :]
    X_ter = np.zeros((B, 9))
    X_ter[:, 0:2] = x_init[:, 0:2] + gait.gait_horizon * gait.gait_period * v_des[:, 0:2]
    X_ter[:, 2] = gait.nom_ht
    X_ter[:, 3:6] = v_des
    X_ter[:, 6:9] = amom
    return X_nom.reshape(B, 9 * H), X_ter


@dataclass
class Batch:
    """Inputs of B independent BiconvexMP solves, harness level."""
    name: str
    B: int
    H: int
    E: int
    m: float
    rho: float
    cnt_plan: np.ndarray       # (B,H,E,4)
    dt: np.ndarray             # (B,H)
    x_init: np.ndarray         # (B,9)
    X_nom: np.ndarray          # (B,9H)
    X_ter: np.ndarray          # (B,9)
    W_X: np.ndarray            # (1 or B, 9H)   tile(W_X, H)
    W_X_ter: np.ndarray        # (1 or B, 9)
    W_F: np.ndarray            # (1 or B, 3EH)  tile(W_F, H)
    bounds: np.ndarray         # (1 or B, H, 6)
    swing_time: np.ndarray = None
    gait_id: np.ndarray = None
    mu: float = 1.0            # friction coefficient of the "SoC" projection (fista.hpp:60)
    meta: dict = field(default_factory=dict)

    def warm_start(self):
        """KinoDynMP::set_warm_starts (kino_dyn.cpp:83-99): X = tile(x0), F = 0, P = 0."""
        X = np.tile(self.x_init, (1, self.H + 1))
        F = np.zeros((self.B, 3 * self.E * self.H))
        P = np.zeros((self.B, 9 * (self.H + 1)))
        return X, F, P

    def take(self, idx):
        """sub-batch of the problems listed in idx"""
        idx = np.asarray(idx)

        def s(a):
            return a if a is None or a.shape[0] == 1 else a[idx]
        return Batch(self.name, len(idx), self.H, self.E, self.m, self.rho, self.cnt_plan[idx],
                     self.dt[idx], self.x_init[idx], self.X_nom[idx], self.X_ter[idx],
                     s(self.W_X), s(self.W_X_ter), s(self.W_F), s(self.bounds),
                     None if self.swing_time is None else self.swing_time[idx],
                     None if self.gait_id is None else self.gait_id[idx], self.mu, dict(self.meta))

    def slice(self, lo, hi):
        def s(a):
            return a if a is None or a.shape[0] == 1 else a[lo:hi]
        return Batch(self.name, hi - lo, self.H, self.E, self.m, self.rho, self.cnt_plan[lo:hi],
                     self.dt[lo:hi], self.x_init[lo:hi], self.X_nom[lo:hi], self.X_ter[lo:hi],
                     s(self.W_X), s(self.W_X_ter), s(self.W_F), s(self.bounds),
                     None if self.swing_time is None else self.swing_time[lo:hi],
                     None if self.gait_id is None else self.gait_id[lo:hi], self.mu, dict(self.meta))


def block_costs(Qx, qx, Qf, E, yaw, lam=0.25):
    """Per-knot block costs from a batch's diagonal raw arrays Qx, qx (B, 9 (H + 1)) and Qf (B, 3 E H): what a heading-aligned cost
    and a force-distribution term look like (tests, tools/block_cost_bench.py).
      * every 3-vector's weights w become R diag(w) R' with R the rotation about z by the problem's yaw (B,) [rad];
      * F gains lam * mean(w of the knot) * kron(Laplacian_E, I_3): the sum over pairs of feet of |f_n - f_m|^2.
    Both parts are positive semi-definite by construction, which is asserted (eigvalsh(block).min() >= -1e-12 eigvalsh(block).max()).
    qx follows the rotated Q: q = -2 Q x_ref with x_ref the reference the diagonal pair (Qx, qx) encodes.
    Returns dict(Qx_blk (B, H + 1, 9, 9), Qf_blk (B, H, 3E, 3E), qx (B, 9 (H + 1)))."""
    Qx, qx, Qf = (np.asarray(a, dtype=np.float64) for a in (Qx, qx, Qf))
    B, K, H = Qx.shape[0], Qx.shape[1] // 9, Qf.shape[1] // (3 * E)
    yaw = np.broadcast_to(np.asarray(yaw, dtype=np.float64), (B,))
    Qx_blk, Qf_blk, q = np.zeros((B, K, 9, 9)), np.zeros((B, H, 3 * E, 3 * E)), np.zeros((B, 9 * K))
    lap = np.kron(E * np.eye(E) - np.ones((E, E)), np.eye(3))
    for i in range(B):
        c, s = np.cos(yaw[i]), np.sin(yaw[i])
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        for t in range(K):
            w = Qx[i, 9 * t:9 * t + 9]
            for g in range(3):
                Qx_blk[i, t, 3 * g:3 * g + 3, 3 * g:3 * g + 3] = R @ np.diag(w[3 * g:3 * g + 3]) @ R.T
        for t in range(H):
            w = Qf[i, 3 * E * t:3 * E * t + 3 * E]
            for n in range(E):
                Qf_blk[i, t, 3 * n:3 * n + 3, 3 * n:3 * n + 3] = R @ np.diag(w[3 * n:3 * n + 3]) @ R.T
            Qf_blk[i, t] += lam * w.mean() * lap
        x_ref = -0.5 * qx[i] / np.where(Qx[i] != 0, Qx[i], 1.0)
        q[i] = -2.0 * np.einsum("tab,tb->ta", (Qx_blk[i] + Qx_blk[i].transpose(0, 2, 1)) / 2, x_ref.reshape(K, 9)).reshape(-1)
    Qx_blk = (Qx_blk + Qx_blk.transpose(0, 1, 3, 2)) / 2      # exactly symmetric
    Qf_blk = (Qf_blk + Qf_blk.transpose(0, 1, 3, 2)) / 2
    for blk in (Qx_blk, Qf_blk):
        ev = np.linalg.eigvalsh(blk)
        assert np.all(ev.min(axis=-1) >= -1e-12 * ev.max(axis=-1)), "block cost is not positive semi-definite"
    return dict(Qx_blk=Qx_blk, Qf_blk=Qf_blk, qx=q)


def block_diag_matrix(blk):
    """The square matrix whose diagonal blocks are blk (n, k, k), dense: what set_cost_x / set_cost_f take"""
    n, k, _ = blk.shape
    Q = np.zeros((n * k, n * k))
    for t in range(n):
        Q[t * k:(t + 1) * k, t * k:(t + 1) * k] = blk[t]
    return Q


def rate_costs(Qx, Qf, E, lam_x, lam_f):
    """Costs between neighbouring knots from a batch's diagonal raw arrays Qx (B, 9 (H + 1)) and Qf (B, 3 E H): a force-rate term
    sum_t (F_{t+1} - F_t)' R_f[t] (F_{t+1} - F_t) with R_f[t] = lam_f * Qf[t], t = 0 .. H - 2, and the same difference on X with
    R_x[t] = lam_x * Qx[t], t = 0 .. H - 1, the three CoM-position components set to 0 (a rate cost on velocity and angular momentum:
    CoM acceleration, momentum rate).  Each is D' R D with D the first difference over the knots: diag[t] += R[t - 1] + R[t],
    off[t] = -R[t] (tests, tools/band_cost_bench.py).
    Returns dict(Qx (B, 9 (H + 1)), Qx_off (B, H, 9), Qf (B, 3 E H), Qf_off (B, H - 1, 3 E))."""
    Qx, Qf = (np.asarray(a, dtype=np.float64) for a in (Qx, Qf))
    B, K, H = Qx.shape[0], Qx.shape[1] // 9, Qf.shape[1] // (3 * E)
    dx, df = Qx.reshape(B, K, 9).copy(), Qf.reshape(B, H, 3 * E).copy()
    Rx, Rf = lam_x * dx[:, :-1], lam_f * df[:, :-1]
    Rx[:, :, :3] = 0.0
    dx[:, :-1] += Rx
    dx[:, 1:] += Rx
    df[:, :-1] += Rf
    df[:, 1:] += Rf
    return dict(Qx=dx.reshape(B, -1), Qx_off=-Rx, Qf=df.reshape(B, -1), Qf_off=-Rf)


def band_matrix(diag, off):
    """The square matrix with diag (n k values) on its diagonal and off (n - 1, k) between the same components of neighbouring
    knots, Q[(t, i), (t + 1, i)] = Q[(t + 1, i), (t, i)] = off[t][i], dense: what set_cost_x / set_cost_f take"""
    off = np.asarray(off, dtype=np.float64)
    k = off.shape[1]
    diag = np.asarray(diag, dtype=np.float64).reshape(-1)
    assert diag.size == (off.shape[0] + 1) * k
    Q = np.diag(diag)
    i = np.arange(off.size)
    Q[i, i + k] = off.reshape(-1)
    Q[i + k, i] = off.reshape(-1)
    return Q


def plane_normals(B, H, E, roll, pitch):
    """Unit normals (B, H, E, 3) of a plane tilted by roll (about world x) and pitch (about world y), radians -- scalars or one value
    per problem: n = R_y(pitch) R_x(roll) e_z, the same for every knot and foot of a problem.  What solve_host / DeviceBatch take as
    cone=dict(projection="euclidean", normals=...): a slope as a workload."""
    roll, pitch = np.broadcast_to(np.asarray(roll, dtype=np.float64), (B,)), np.broadcast_to(np.asarray(pitch, dtype=np.float64), (B,))
    n = np.stack([np.sin(pitch) * np.cos(roll), -np.sin(roll), np.cos(pitch) * np.cos(roll)], axis=-1)
    return np.ascontiguousarray(np.broadcast_to(n[:, None, None, :], (B, H, E, 3)))


def _draws(seed, first, B, n):
    """Per-problem independent streams: problem b always sees the same numbers whatever the
    batch size or the rank that generates it (SeedSequence.spawn keyed by absolute index)."""
    out_u = np.empty((B, n))
    out_n = np.empty((B, n))
    for b in range(B):
        g = np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, first + b])))
        out_u[b] = g.random(n)
        out_n[b] = g.standard_normal(n)
    return out_u, out_n


def make_batch(config, B, first=0, seed=None, H=None, height_map=None):
    """SURVEY.md 8d configs.
      "solo12_trot_nominal"  config 1 (every problem identical, B usually 1)
      "solo12_trot"          config 2 perturbed ICs
      "go2_bound"            config 3 (synthetic robot), H forced to 40, nom_ht 0.30, mu = 10:
                             with the reference's fixed mu = 1 its squared-norm "SoC" projection
                             blows up for a 15 kg robot (tests/test_oracle_cpu.py) -- the one
                             parameter a Go2 user would have to change (set_friction_coefficient,
                             biconvex.hpp:131)
      "solo12_mixed"         config 4 trot/bound/pace with per-problem weights, H = 20
      "biped_walk"           synthetic biped (BIPED, n_eff = 2), walk / hop mix with per-problem weights (W_F: 6 per knot),
                             H = 20, mu = BIPED_MU; draws as "solo12_trot"
    `first` = absolute index of problem 0 (for rank sharding).
    height_map: the terrain the contact plan is built on (contact_plan explains it; kept in meta, None: flat ground).  With one
    terrain per problem, problem b of the batch has terrain b."""
    cfg_index = {"solo12_trot_nominal": 1, "solo12_trot": 2, "go2_bound": 3, "solo12_mixed": 4, "biped_walk": 6}[config]
    seed = BASE_SEED + cfg_index if seed is None else seed
    robot = GO2 if config == "go2_bound" else (BIPED if config == "biped_walk" else SOLO12)
    E = robot.feet_xy.shape[0]
    if config == "biped_walk":
        gaits = [BIPED_WALK, BIPED_HOP]
        H = BIPED_WALK.horizon if H is None else H
    elif config == "solo12_mixed":
        gaits = [TROT, BOUND, PACE]
        H = 20 if H is None else H
    elif config == "go2_bound":
        gaits = [replace(BOUND, nom_ht=0.30)]
        H = 40 if H is None else H
    else:
        gaits = [TROT]
        H = TROT.horizon if H is None else H
    u, nrm = _draws(seed, first, B, 32)
    x_init = np.zeros((B, 9))
    x_init[:, 2] = robot.com_height
    v_des = np.zeros((B, 3))
    feet0 = np.zeros((B, E, 3))
    feet0[:, :, 0:2] = robot.feet_xy[None]
    feet0[:, :, 2] = FOOT_SIZE
    if config == "solo12_trot_nominal":
        t0 = np.zeros(B)
        v_des[:, 0] = 0.2
        gid = np.zeros(B, dtype=np.int64)
    else:
        t0 = np.round(0.05 * np.floor(u[:, 0] * 10), 3)
        v_des[:, 0] = 0.3 * u[:, 1]
        gid = np.minimum((u[:, 2] * len(gaits)).astype(np.int64), len(gaits) - 1)
        x_init[:, 0:3] += nrm[:, 0:3] * np.array([0.02, 0.02, 0.01])
        x_init[:, 3:6] += nrm[:, 3:6] * 0.1
        x_init[:, 6:9] += nrm[:, 6:9] * 0.02
        feet0[:, :, 0:2] += 0.01 * nrm[:, 9:9 + 2 * E].reshape(B, E, 2)
    feet0_raw = feet0.copy()
    feet0 = np.round(feet0, 3)                       # :215 np.round(oMf.translation, 3)
    com_xy = np.round(x_init[:, 0:2], 3)             # :164
    w_des = np.zeros(B)
    cnt = np.zeros((B, H, E, 4))
    swing = np.zeros((B, H, E))
    dt = np.zeros((B, H))
    X_nom = np.zeros((B, 9 * H))
    X_ter = np.zeros((B, 9))
    for k, g in enumerate(gaits):
        sel = np.nonzero(gid == k)[0]
        if sel.size == 0:
            continue
        c, s, d = contact_plan(g, robot, H, t0[sel], com_xy[sel], x_init[sel, 2], feet0[sel],
                               v_des[sel], w_des[sel], height_map=height_map, problem=sel)
        cnt[sel], swing[sel], dt[sel] = c, s, d
        X_nom[sel], X_ter[sel] = centroidal_costs(g, H, x_init[sel], v_des[sel], d)
    if len(gaits) == 1:
        g = gaits[0]
        W_X = np.tile(g.W_X, H)[None]
        W_X_ter = g.W_X_ter[None].copy()
        W_F = np.tile(g.W_F, H)[None]
    else:
        W_X = np.stack([np.tile(gaits[k].W_X, H) for k in gid])
        W_X_ter = np.stack([gaits[k].W_X_ter for k in gid])
        W_F = np.stack([np.tile(gaits[k].W_F, H) for k in gid])
    bounds = np.tile(BOUNDS_TILE, (H, 1))[None]
    return Batch(config, B, H, E, robot.mass, gaits[0].rho, cnt, dt, x_init, X_nom, X_ter,
                 W_X, W_X_ter, W_F, bounds, swing, gid, {"go2_bound": 10.0, "biped_walk": BIPED_MU}.get(config, 1.0),
                 dict(seed=seed, first=first, t0=t0, v_des=v_des, gaits=[g.name for g in gaits], gait_objs=gaits, robot=robot,
                      feet0_raw=feet0_raw, w_des=w_des, height_map=height_map))


# ------------------------------------------------------------------- whole-body batches ---
SOLO12_Q0 = np.array([0, 0, 0.2409, 0, 0, 0, 1] + [0, 0.8, -1.6] * 2 + [0, -0.8, 1.6] * 2, float)  # feet at z = foot_size
FEET = ("FL_FOOT", "FR_FOOT", "HL_FOOT", "HR_FOOT")     # abstract_cyclic_gen.py:37
HIPS = ("FL_HFE", "FR_HFE", "HL_HFE", "HR_HFE")         # abstract_cyclic_gen.py:38


@dataclass
class WholeBodyRobot:
    """What the harness constructor reads from a robot_properties config (abstract_cyclic_gen.py:28-76)"""
    name: str
    q0: np.ndarray             # nominal configuration (feet on the ground)
    feet: tuple                # eff_names
    hips: tuple                # hip_names
    mu: float = 1.0            # friction coefficient of the force projection (fista.hpp:49: 1.0 in the reference)


SOLO12_WB = WholeBodyRobot("solo12", SOLO12_Q0, FEET, HIPS)
# synthetic: robot_properties_go2/config.py:108-113,162-165 names / joint angles,
# base lowered from 0.35 so the feet rest at z = foot radius 0.02
GO2_Q0 = np.array([0, 0, 0.3168, 0, 0, 0, 1] + [0, 0.8, -1.6] * 4, float)
GO2_WB = WholeBodyRobot("go2", GO2_Q0, ("FL_foot", "FR_foot", "RL_foot", "RR_foot"),
                        ("FL_thigh_joint", "FR_thigh_joint", "RL_thigh_joint", "RR_thigh_joint"), mu=10.0)
# IK weights of the trot plan (motions/cyclic/solo12_trot.py:22-31)
TROT_IK = dict(state_wt=np.array([0., 0, 10] + [1000] * 3 + [1.0] * 12 + [0.] * 3 + [100] * 3 + [0.5] * 12),
               ctrl_wt=np.array([0, 0, 1000] + [5e2] * 3 + [1.0] * 12), swing_wt=(1e4, 1e4), cent_wt=(0.0, 5e2),
               reg_wt=(5e-2, 1e-5))
# IK weights of the turning trot (motions/cyclic/solo12_trot.py:55-64): the yaw entries of state_wt 10 in place of 1000 and 100
TROT_TURN_IK = dict(TROT_IK, state_wt=np.array([0., 0, 10] + [1000, 1000, 10] + [1.0] * 12 + [0.] * 3 + [100, 100, 10] + [0.5] * 12))


@dataclass
class WholeBodyBatch:
    """Inputs of B independent KinoDynMP.optimize(q, v, N, 1) calls as the harness prepares them."""
    dyn: Batch                 # centroidal part (x_init = [com, vcom, L] of (q, v))
    x: np.ndarray              # (B,37) [q, v]
    ik_T: int
    ik_tasks: np.ndarray       # (B, T+1, 33) kernel task blocks; com/mom refs are filled after the ADMM
    state_w: np.ndarray        # (1,36)
    ctrl_w: np.ndarray         # (1,18)
    x_reg: np.ndarray          # (B,37)
    wt_com: float
    wt_mom: float
    frame_ids: tuple

    def take(self, idx):
        """sub-batch of the problems listed in idx (copies)"""
        idx = np.asarray(idx)
        return WholeBodyBatch(self.dyn.take(idx), self.x[idx].copy(), self.ik_T, self.ik_tasks[idx].copy(), self.state_w, self.ctrl_w,
                              self.x_reg[idx].copy(), self.wt_com, self.wt_mom, self.frame_ids)


def _log3_batch(R):
    v = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    t = np.arctan2(0.5 * np.linalg.norm(v, axis=1), 0.5 * (np.trace(R, axis1=1, axis2=2) - 1.0))
    f = np.where(t < 1e-3, 0.5 * (1 + t * t / 6 + 7 * t ** 4 / 360), t / (2 * np.sin(np.where(t < 1e-3, 1.0, t))))
    w = f[:, None] * v
    c = 0.5 * (np.trace(R, axis1=1, axis2=2) - 1.0)
    for b in np.nonzero(c < -0.5)[0]:      # beyond 2 pi / 3 the axis from the symmetric part, as rbd::log3 takes it: a a^T = (sym R - c I)/(1 - c)
        d = (np.diag(R[b]) - c[b]) / (1.0 - c[b])
        k = int(np.argmax(d))
        ax = 0.5 * (R[b][:, k] + R[b][k, :]) / ((1.0 - c[b]) * np.sqrt(d[k]))
        ax[k] = np.sqrt(d[k])
        w[b] = (-t[b] if ax @ v[b] < 0 else t[b]) * ax
    return w


def make_wb_batch(model, B, first=0, seed=None, gait=TROT, ik=TROT_IK, ik_hor_ratio=0.5, wb=None, height_map=None, w_des=None):
    """Perturbed whole-body states and everything SoloMpcGaitGen.optimize hands to KinoDynMP
    (abstract_cyclic_gen.py:629-663): contact plan from the feet / CoM of (q, v), centroidal costs
    (create_costs :564-614) and the IK task list (:545-562).  Solo12 trot by default.  height_map: the terrain of the contact
    plan (contact_plan explains it; kept in meta); the via-point height step_ht and nom_ht stay absolute, as in the reference.
    w_des (B,): desired yaw rates.  A problem with w_des != 0 takes the reference's turning branch: centrifugal steps (:285-286),
    ori_des = q[3:7] (:636-639) and the yaw-momentum reference yaw_inertia * w_des (:602-607), yaw_inertia =
    composite_inertia_base(model, q0)[2, 2] (kept in meta); None or zeros: the arrays without it, bit for bit."""
    Q0 = (SOLO12_WB if wb is None else wb).q0
    seed = BASE_SEED + 5 if seed is None else seed
    u, nrm = _draws(seed, first, B, 48)
    # state perturbation in the tangent space of q0
    dq = np.zeros((B, 18))
    dq[:, 2] = 0.01 * nrm[:, 0]
    dq[:, 3:6] = 0.05 * nrm[:, 1:4]
    dq[:, 6:] = 0.05 * nrm[:, 4:16]
    q = np.tile(Q0, (B, 1))
    q[:, 2] += dq[:, 2]
    # small rotation: quaternion of exp(w)
    w = dq[:, 3:6]
    th = np.linalg.norm(w, axis=1)
    sfac = np.where(th < 1e-8, 0.5, np.sin(0.5 * th) / np.where(th < 1e-8, 1.0, th))
    q[:, 3:6] = sfac[:, None] * w
    q[:, 6] = np.cos(0.5 * th)
    q[:, 7:] += dq[:, 6:]
    v = np.concatenate([0.1 * nrm[:, 16:19], 0.2 * nrm[:, 19:22], 0.2 * nrm[:, 22:34]], axis=1)
    t0 = np.round(0.05 * np.floor(u[:, 0] * 10), 3)
    v_des_b = np.zeros((B, 3))
    v_des_b[:, 0] = 0.3 * u[:, 1]
    return wb_batch_of_states(model, q, v, t0, v_des_b, gait, ik, ik_hor_ratio, wb, height_map, w_des, dict(seed=seed, first=first))


def wb_batch_of_states(model, q, v, t0, v_des_b, gait=TROT, ik=TROT_IK, ik_hor_ratio=0.5, wb=None, height_map=None, w_des=None, meta=None):
    """make_wb_batch for the caller's states q (B,19) (base x, y as SoloMpcGaitGen.optimize leaves them: 0), v (B,18), times t0 (B,)
    and body-frame desired velocities v_des_b (B,3); meta: what the batch's meta should hold beside the inputs"""
    from . import fk_np
    wb = SOLO12_WB if wb is None else wb
    Q0, FEET, HIPS = wb.q0, wb.feet, wb.hips
    B, E, H = q.shape[0], 4, gait.horizon
    T = int(np.round(ik_hor_ratio * gait.gait_horizon * gait.gait_period / gait.gait_dt, 2))   # :128
    kin = fk_np.kinematics(model, q, v)
    Rb = kin["oR"][0]
    v_des = np.einsum("bij,bj->bi", Rb, v_des_b)                    # :642-643
    # constructor offsets from the nominal configuration (:41-76)
    k0 = fk_np.kinematics(model, Q0[None])
    offs = np.round(fk_np.frame_positions(model, k0, HIPS)[0] - k0["com"][0], 3)
    offs[:, 1] += np.array([0.04, -0.04, 0.04, -0.04])
    yaw = np.arctan2(Rb[:, 1, 0], Rb[:, 0, 0])
    cy, sy = np.cos(yaw), np.sin(yaw)
    hip_off = np.stack([cy[:, None] * offs[None, :, 0] - sy[:, None] * offs[None, :, 1],
                        sy[:, None] * offs[None, :, 0] + cy[:, None] * offs[None, :, 1]], axis=2)   # (B,4,2)
    feet0 = np.round(fk_np.frame_positions(model, kin, FEET), 3)
    com_xy = np.round(kin["com"][:, 0:2], 3)
    robot = RobotParams(wb.name, model.total_mass, fk_np.frame_positions(model, k0, FEET)[0][:, 0:2], offs[:, 0:2],
                        float(k0["com"][0, 2]))
    w_des = np.zeros(B) if w_des is None else np.array(w_des, dtype=np.float64).reshape(B)
    turning = w_des != 0                                              # the reference's test (:603, :636): a NaN turns
    cnt, swing, dt = contact_plan(gait, robot, H, t0, com_xy, kin["com"][:, 2], feet0, v_des, w_des, hip_off, height_map=height_map)
    x_init = np.concatenate([kin["com"], kin["vcom"], kin["L"]], axis=1)
    amom = _log3_batch(np.transpose(Rb, (0, 2, 1)))                   # log3(R_des R_q^T), R_des = I  (:616-627)
    yaw_inertia = None
    if turning.any():
        from .cyclic_gen import composite_inertia_base
        yaw_inertia = float(composite_inertia_base(model, Q0)[2, 2])  # rdata.Ycrb[1].inertia of q0 (:48-49)
        z, o = np.zeros(B), np.ones(B)
        R_des = np.stack([np.stack([cy, -sy, z], axis=1), np.stack([sy, cy, z], axis=1), np.stack([z, z, o], axis=1)], axis=1)   # :588-591
        amom = np.where(turning[:, None], _log3_batch(R_des @ np.transpose(Rb, (0, 2, 1))), amom)
    X_nom, X_ter = centroidal_costs(gait, H, x_init, v_des, dt, amom)
    if turning.any():                                                 # :602-607
        X_nom[turning, 8::9] = (yaw_inertia * w_des[turning])[:, None]
        X_ter[turning, 8] = yaw_inertia * w_des[turning]
    dyn = Batch(wb.name + "_" + gait.name + "_wb", B, H, E, model.total_mass, gait.rho, cnt, dt, x_init, X_nom, X_ter,
                np.tile(gait.W_X, H)[None], gait.W_X_ter[None].copy(), np.tile(gait.W_F, H)[None],
                np.tile(BOUNDS_TILE, (H, 1))[None], swing, np.zeros(B, dtype=np.int64), wb.mu,
                dict(meta or {}, t0=t0, v_des=v_des, v_des_body=v_des_b, height_map=height_map, w_des=w_des, yaw_inertia=yaw_inertia))
    # IK task blocks: 4 x {w, frame, ref3} | com {w, ref3} | mom {w, ref6} | state w | ctrl w
    fid = tuple(model.frame_id(n) for n in FEET)
    tasks = np.zeros((B, T + 1, 33))
    for i in range(T):
        for j in range(E):
            on = cnt[:, i, j, 0] == 1
            via = (~on) & (swing[:, i, j] == 1)
            ref = cnt[:, i, j, 1:4].copy()
            ref[via, 2] = gait.step_ht
            tasks[:, i, 5 * j] = np.where(on, ik["swing_wt"][0], np.where(via, ik["swing_wt"][1], 0.0))
            tasks[:, i, 5 * j + 1] = fid[j]
            tasks[:, i, 5 * j + 2:5 * j + 5] = ref
    tasks[:, :, 20] = ik["cent_wt"][0]
    tasks[:, :, 24] = ik["cent_wt"][1]
    tasks[:, :, 31] = ik["reg_wt"][0]
    tasks[:, :, 32] = ik["reg_wt"][1]
    x = np.concatenate([q, v], axis=1)
    x_reg = np.concatenate([np.tile(Q0, (B, 1)), np.zeros((B, 18))], axis=1)
    return WholeBodyBatch(dyn, x, T, tasks, ik["state_wt"][None].copy(), ik["ctrl_wt"][None].copy(), x_reg,
                          ik["cent_wt"][0], ik["cent_wt"][1], fid)
