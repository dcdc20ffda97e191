"""The twin of the device-side acyclic plan (include/ext/bunmpc_acyclic.h): bunmpc_amd.acyclic_gen.SoloAcyclicGen itself, driven with
recording stand-ins for its solver objects, and what they receive packed into the arrays of bmpc_acyclic_plan_t -- so the spec the
device is held to is the mirror's own code, call by call.  No GPU.  Also hold_np, the zero-order-hold expansion of its optimize, and
hop_plan, the synthetic motion table of the tests (our own numbers, in the shape of motions/weight_abstract.py::ACyclicMotionParams).
The mirror itself is held to a recording of the reference's generator on the reference's own tables (tests/golden/acyclic/acyclic_ref.npz):
pack_table / unpack_table / ref_cases read and write that file's tables and cases."""
import types

import numpy as np

from bunmpc_amd import problems
from bunmpc_amd.acyclic_gen import SoloAcyclicGen

FRAME_SLOTS = 1      # BMPC_ACY_FRAME_SLOTS


def hop_plan(swing=(0.35, 0.45), swing_feet=(1, 1, 1, 1)):
    """A hop: stance [0, 0.3), flight [0.3, 0.5), landing [0.5, 0.9) with the feet 5 cm ahead; three rows of nominal states, two of
    bounds, one swing window (inside the flight; the variant of the slot test lets it start in the stance), two state and two control
    phases that switch at 0.5 with different weights and scales."""
    q0 = problems.SOLO12_Q0.copy()
    q_tuck = q0.copy()
    q_tuck[2] += 0.06
    q_tuck[7:] = np.array([0, 1.1, -2.2] * 2 + [0, -1.1, 2.2] * 2)
    feet = np.array([[0.195, 0.147, 0.018], [0.195, -0.147, 0.018], [-0.195, 0.147, 0.018], [-0.195, -0.147, 0.018]])
    ahead = feet + np.array([0.05, 0.0, 0.0])
    p = types.SimpleNamespace()
    p.n_col, p.dt_arr, p.plan_freq = 12, np.full(12, 0.05), [[0.3, 0, 0.9]]
    p.cnt_plan = [[[1.0, *feet[j], 0.0, 0.3] for j in range(4)], [[0.0, *feet[j], 0.3, 0.5] for j in range(4)],
                  [[1.0, *ahead[j], 0.5, 0.9] for j in range(4)]]
    p.W_X = np.array([2e-5, 1e-5, 8e4, 1e1, 1e1, 3e2, 1e4, 2e4, 1e4])
    p.W_X_ter = 8 * p.W_X
    p.W_F = np.array(4 * [2e1, 1e1, 1e1])
    p.rho = 4e4
    p.X_nom = [[0, 0, 0.2, 0, 0, 0, 0, 0, 0, 0.0, 0.3], [0.02, 0, 0.3, 0.25, 0, 0, 0, 0, 0, 0.3, 0.5], [0.05, 0, 0.21, 0, 0, 0, 0, 0, 0, 0.5, 0.9]]
    p.X_ter = np.array([0.05, 0, 0.22, 0, 0, 0, 0, 0, 0.0])
    p.bounds = [[-0.25, -0.25, 0.1, 0.25, 0.25, 0.3, 0.0, 0.5], [-0.2, -0.2, 0.12, 0.2, 0.2, 0.28, 0.5, 0.9]]
    # (momentum weight 4: with 40 the DDP of the case before the motion's start, whose first two nodes carry no state and no control
    # cost, creeps -- 100 iterations and still |Q_u|^2 = 1.3e-6, through the single-problem handle and through the batch alike)
    p.cnt_wt, p.cent_wt = 1.2e3, [2e-1, 4e0]
    p.swing_wt = [[[4e2 * swing_feet[j], feet[j][0] + 0.02, feet[j][1], 0.09, swing[0], swing[1]] for j in range(4)]]
    sw1 = np.array([0., 0, 10] + [900] * 3 + [1.0] * 12 + [0.] * 3 + [90] * 3 + [0.5] * 12)
    sw2 = np.array([0., 0, 80] + [450] * 3 + [8.0] * 12 + [0.] * 3 + [110] * 3 + [1.0] * 12)
    p.state_reg = [np.hstack([q_tuck, np.zeros(18), 0.0, 0.5]), np.hstack([q0, np.zeros(18), 0.5, 0.9])]
    p.state_wt = [np.hstack([sw1, 0.0, 0.5]), np.hstack([sw2, 0.5, 0.9])]
    p.state_scale = [[1e-2, 0.0, 0.5], [4e-2, 0.5, 0.9]]
    cw = np.array([1e-2, 0, 900] + [4e2] * 3 + [1.0] * 12)
    p.ctrl_wt = [np.hstack([cw, 0.0, 0.5]), np.hstack([3 * cw, 0.5, 0.9])]
    p.ctrl_reg = [np.hstack([np.zeros(18), 0.0, 0.5]), np.hstack([np.zeros(18), 0.5, 0.9])]
    p.ctrl_scale = [[1e-4, 0.0, 0.5], [3e-4, 0.5, 0.9]]
    p.kp, p.kd = [[2.5, 0.0, 0.9]], [[0.08, 0.0, 0.9]]
    return p


def slot_plan():
    """the hop with a swing window that starts inside the stance and only FL swinging: at those nodes FL is in contact and has a swing
    task -- five frame tasks"""
    return hop_plan(swing=(0.2, 0.45), swing_feet=(1, 0, 0, 0))


# motion times t - t0 of the tests (t0 = 0), and one case with t0 != 0 and an off-grid absolute t: remainder(0.37, 0.05) = 0.02 gives
# dt[0] = 0.03, where t - t0 = 0.15 would give 0.05
TIMES = [(0.0, 0.0), (0.02, 0.0), (0.05, 0.0), (0.27, 0.0), (0.3, 0.0), (0.45, 0.0), (0.6, 0.0), (0.88, 0.0), (0.95, 0.0), (1.5, 0.0), (-0.1, 0.0), (0.37, 0.22)]


def states():
    """the nominal state and a perturbed one, (2, 37)"""
    rng = np.random.default_rng(20240607)
    x = np.zeros((2, 37))
    x[:, :19] = problems.SOLO12_Q0
    x[1, 0:3] += rng.normal(0, 0.01, 3)
    quat = x[1, 3:7] + rng.normal(0, 0.03, 4)
    x[1, 3:7] = quat / np.linalg.norm(quat)
    x[1, 7:19] += rng.normal(0, 0.05, 12)
    x[1, 19:] = rng.normal(0, 0.1, 18)
    return x


def cases():
    """x (24, 37), t (24,), t0 (24,): every time of TIMES with both states"""
    xs = states()
    x = np.concatenate([xs[s][None] for _ in TIMES for s in range(2)])
    t = np.array([tt for tt, _ in TIMES for _ in range(2)])
    t0 = np.array([t00 for _, t00 in TIMES for _ in range(2)])
    return x, t, t0


class _Mp:
    def __init__(self):
        self.cnt, self.dt = [], []

    def set_rho(self, rho): pass

    def set_contact_plan(self, cnt, dt):
        self.cnt.append(np.array(cnt, dtype=np.float64))
        self.dt.append(float(dt))

    def create_bound_constraints(self, b, fx, fy, fz): self.bounds = np.array(b, dtype=np.float64)

    def create_cost_X(self, W_X, W_X_ter, X_ter, X_nom): self.X_ter, self.X_nom = np.array(X_ter, dtype=np.float64), np.array(X_nom, dtype=np.float64)

    def create_cost_F(self, W_F): pass


class _Ik:
    """the node blocks of bmpc_ik_batch_t.tasks as the calls arrive; frame tasks in call order, the first four kept"""

    def __init__(self, T):
        self.T = T
        self.tasks, self.state_w, self.ctrl_w = np.zeros((T + 1, 33)), np.zeros((T + 1, 36)), np.zeros((T, 18))
        self.x_reg = np.zeros((T + 1, 37))
        self.x_reg[:, 6] = 1.0      # a node without the cost keeps the neutral reference
        self.frames = [0] * (T + 1)

    def add_position_tracking_task_single(self, fid, ref, wt, name, i):
        assert 0 <= i < self.T
        if self.frames[i] < 4:
            self.tasks[i, 5 * self.frames[i]:5 * self.frames[i] + 5] = [wt, fid, *ref]
        self.frames[i] += 1

    def _state(self, i, wt, wts, ref):
        assert self.tasks[i, 31] == 0 and len(wts) == 36 and len(ref) == 37
        self.tasks[i, 31], self.state_w[i], self.x_reg[i] = wt, wts, ref

    def add_state_regularization_cost_single(self, i, wt, name, wts, ref):
        assert i < self.T
        self._state(i, wt, wts, ref)

    def add_state_regularization_cost(self, sn, en, wt, name, wts, ref, terminal):
        assert terminal and en == self.T
        self._state(self.T, wt, wts, ref)

    def add_ctrl_regularization_cost_single(self, i, wt, name, wts, ref):
        assert i < self.T and self.tasks[i, 32] == 0 and len(wts) == 18
        self.tasks[i, 32], self.ctrl_w[i] = wt, wts

    def add_ctrl_regularization_cost(self, sn, en, wt, name, wts, ref, terminal):
        assert terminal and en == self.T
        self.tasks[self.T, 32] = wt      # the terminal node has no control: the weight is recorded, the vector has no row

    def setup_costs(self, dt): self.dt = np.array(dt, dtype=np.float64)


class _Kd:
    def __init__(self, T):
        self.mp, self.ik = _Mp(), _Ik(T)

    def set_com_tracking_weight(self, w): self.wt_com = float(np.asarray(w).reshape(-1)[0])

    def set_mom_tracking_weight(self, w): self.wt_mom = float(np.asarray(w).reshape(-1)[0])

    def return_ik(self): return self.ik

    def return_dyn(self): return self.mp


def _shared_last_row(plan):
    """the planted fault: `plan` as the rule "row len(state_reg) - 1 of state_wt, state_reg and state_scale past the end" (and row
    len(ctrl_scale) - 1 of the control lists) sees it.  Inside a table only rows below that count are read, so cutting the longer
    lists to it changes nothing but what each list's last row is."""
    cut = types.SimpleNamespace(**vars(plan))
    ns, nc = len(plan.state_reg), len(plan.ctrl_scale)
    cut.state_wt, cut.state_scale, cut.ctrl_wt, cut.ctrl_reg = plan.state_wt[:ns], plan.state_scale[:ns], plan.ctrl_wt[:nc], plan.ctrl_reg[:nc]
    return cut


def plan_np(model, plan, x, t, t0, fault=None):
    """the arrays of bmpc_acyclic_plan_t for one problem, from SoloAcyclicGen.create_contact_plan / create_costs.  `fault` (None in
    every checker) plants one fault for the test that shows the recording has teeth: "shared_last_row"."""
    assert fault in (None, "shared_last_row")
    if fault == "shared_last_row":
        plan = _shared_last_row(plan)
    gen = SoloAcyclicGen(model, model)
    kd = _Kd(plan.n_col)
    gen._make_kd = lambda: kd
    gen.update_motion_params(plan, x[:19], float(t0))
    gen.create_contact_plan(x[:19].copy(), x[19:].copy(), float(t))
    gen.create_costs(x[:19].copy(), x[19:].copy(), float(t))
    H = plan.n_col
    tasks = kd.ik.tasks
    tasks[:, 20], tasks[:, 24] = kd.wt_com, kd.wt_mom      # kino_dyn.cpp:50-56: every node, the terminal one too
    assert len(kd.mp.cnt) == H and np.array_equal(kd.ik.dt[:H], np.asarray(plan.dt_arr)[:H])
    return dict(cnt_plan=np.array(kd.mp.cnt), dt=np.array(kd.mp.dt), dt_ik=kd.ik.dt[:H].copy(), x_init=kd.mp.X_nom[0:9].copy(), X_nom=kd.mp.X_nom,
                X_ter=kd.mp.X_ter, bounds=kd.mp.bounds, ik_tasks=tasks, state_w=kd.ik.state_w, x_reg=kd.ik.x_reg, ctrl_w=kd.ik.ctrl_w,
                status=np.int32(FRAME_SLOTS if max(kd.ik.frames) > 4 else 0), frames=np.array(kd.ik.frames))


def plan_batch_np(model, plan, x, t, t0):
    """plan_np of every problem, stacked; x is kept beside the outputs (what DeviceAcyclicPlan.load_host takes)"""
    rows = [plan_np(model, plan, x[b], t[b], t0[b]) for b in range(len(t))]
    out = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    out["x"] = np.array(x, dtype=np.float64)
    return out


# ---- the recording of the reference's generator (tests/golden/acyclic/acyclic_ref.npz, written by tests/golden/make_golden_acyclic.py) ----

REF_TABLES = ("plan_jump", "rearing", "rearing_jump", "plan_cartwheel", "plan_hifive")
# the time tables of an ACyclicMotionParams: lists of rows, each list with a row count of its own
TABLE_LISTS = ("plan_freq", "cnt_plan", "X_nom", "bounds", "state_reg", "state_wt", "state_scale", "ctrl_wt", "ctrl_reg", "ctrl_scale", "kp", "kd")
TABLE_VECTORS = ("dt_arr", "W_X", "W_X_ter", "W_F", "X_ter", "cent_wt")
TABLE_SCALARS = ("rho", "cnt_wt")
SWING_NONE, SWING_SCALAR, SWING_LIST = 0, 1, 2
STATE_NOMINAL, STATE_PERTURBED, STATE_PLACED = 0, 1, 2      # states(); PLACED: the perturbed state at the reference's initial base position
# what the reference's create_contact_plan / create_costs hand the solver objects, in plan_np's layout, and what the tests compare
REF_OUTPUTS = ("cnt_plan", "dt", "dt_ik", "X_nom", "X_ter", "bounds", "ik_tasks", "state_w", "x_reg", "ctrl_w", "frames")
# int((k / 1000) / 0.001) == k - 1 in IEEE double: the intervals at which a hold count that is not a correctly rounded division differs
HOLD_EDGES_MS = (43, 51, 59, 71, 86, 87)


def pack_table(plan):
    """every field of an ACyclicMotionParams as arrays {field: array}: the lists with `<field>_rows`, swing_wt with a flag"""
    out = dict(n_col=np.int64(plan.n_col), robot_name=np.array(plan.robot_name), motion_name=np.array(plan.motion_name))
    for k in TABLE_LISTS:
        out[k] = np.array([np.asarray(r, dtype=np.float64) for r in getattr(plan, k)], dtype=np.float64)
        out[k + "_rows"] = np.int64(len(getattr(plan, k)))
    for k in TABLE_VECTORS:
        out[k] = np.asarray(getattr(plan, k), dtype=np.float64)
    for k in TABLE_SCALARS:
        out[k] = np.float64(getattr(plan, k))
    sw = plan.swing_wt
    if isinstance(sw, (np.ndarray, list)):
        out["swing_wt_kind"], out["swing_wt"], out["swing_wt_rows"] = np.int64(SWING_LIST), np.asarray(sw, dtype=np.float64), np.int64(len(sw))
    else:
        out["swing_wt_kind"], out["swing_wt_rows"] = np.int64(SWING_NONE if sw is None else SWING_SCALAR), np.int64(0)
        out["swing_wt"] = np.float64(0.0 if sw is None else sw)
    return out


def unpack_table(z, name):
    """the table `name` of the recording as an ACyclicMotionParams-shaped object, from the file alone"""
    g = lambda k: z["%s__%s" % (name, k)]      # noqa: E731
    p = types.SimpleNamespace(n_col=int(g("n_col")), robot_name=str(g("robot_name")), motion_name=str(g("motion_name")))
    for k in TABLE_LISTS:
        rows = g(k)
        assert rows.shape[0] == int(g(k + "_rows"))
        setattr(p, k, [np.array(r) for r in rows])
    for k in TABLE_VECTORS:
        setattr(p, k, np.array(g(k)))
    for k in TABLE_SCALARS:
        setattr(p, k, float(g(k)))
    kind = int(g("swing_wt_kind"))
    p.swing_wt = None if kind == SWING_NONE else float(g("swing_wt")) if kind == SWING_SCALAR else [np.array(r) for r in g("swing_wt")]
    return p


def ref_cases(z, name):
    """the recorded cases of one table: x (B, 37), t (B,), t0 (B,), the recorded x_init (B, 9) -- an INPUT of the recording, from
    oracle/rbd_np.py, not the reference's -- and the arrays the reference's solver objects received"""
    g = lambda k: z["%s__%s" % (name, k)]      # noqa: E731
    return dict(x=g("x"), t=g("t"), t0=g("t0"), kind=g("state_kind"), x_init=g("x_init"), size=g("size"), ref={k: g("out_" + k) for k in REF_OUTPUTS})


def hold_edge_problems():
    """the dt rows of the hold's edge intervals (B = 8, 12 intervals): one problem per edge value as dt[0], one with all six in a
    row, one with 0.04 -- and seeded knots (8, 13, 37)"""
    dt = np.full((len(HOLD_EDGES_MS) + 2, 12), 0.05)
    for b, k in enumerate(HOLD_EDGES_MS):
        dt[b, 0] = k / 1000
    dt[len(HOLD_EDGES_MS), 3:3 + len(HOLD_EDGES_MS)] = [k / 1000 for k in HOLD_EDGES_MS]
    dt[len(HOLD_EDGES_MS) + 1, :] = 0.04
    return np.random.default_rng(8687).normal(size=(len(dt), 13, 37)), dt


def hold_np(knots, dt, size, max_rows=None, step=0.001):
    """SoloAcyclicGen.optimize's expansion (:331-345) of one problem: vstack_i tile(knots[i], int(dt[i] / step)), clipped at max_rows"""
    n = [int(dt[i] / step) for i in range(size)]
    out = np.vstack([np.tile(knots[i], (n[i], 1)) for i in range(size)])
    return out if max_rows is None else out[:max_rows]
