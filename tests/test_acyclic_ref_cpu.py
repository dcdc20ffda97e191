"""The acyclic mirror (bunmpc_amd/acyclic_gen.py, through the twin of tests/acyclic_np.py) against a recording of the REFERENCE's own
generator on its own motion tables (tests/golden/acyclic/acyclic_ref.npz, written by tests/golden/make_golden_acyclic.py): every array
the solver objects receive, bit for bit, on plan_jump, rearing, rearing_jump, plan_cartwheel and plan_hifive.  The tables are rebuilt
from the file alone; only the last test looks for the reference, to run the generator again, and skips where it is not there."""
import importlib.util
import os

import numpy as np
import pytest

from bunmpc_amd import problems, urdf_model
from bunmpc_amd.acyclic_gen import SoloAcyclicGen
from tests import acyclic_np as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBOT = os.path.join(ROOT, "bunmpc_amd", "robots", "solo12.json")
GOLDEN = os.path.join(ROOT, "tests", "golden", "acyclic", "acyclic_ref.npz")
GENERATOR = os.path.join(ROOT, "tests", "golden", "make_golden_acyclic.py")


@pytest.fixture(scope="module")
def model():
    return urdf_model.RobotModel.from_json(open(ROBOT).read())


@pytest.fixture(scope="module")
def rec():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def mirror(model, rec, name, fault=None):
    """plan_np of every recorded case of one table, stacked"""
    c = twin.ref_cases(rec, name)
    plan = twin.unpack_table(rec, name)
    rows = [twin.plan_np(model, plan, c["x"][b], c["t"][b], c["t0"][b], fault=fault) for b in range(len(c["t"]))]
    return c, {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def past_the_state_end(rec, name):
    """(case, node) -> whether the node's time, as the recording's own x_reg / state_w rows show it, is past state_reg's end: the
    rounded walk of the mirror on the recorded t, t0 and dt_arr"""
    c, plan = twin.ref_cases(rec, name), twin.unpack_table(rec, name)
    T, end = plan.n_col, plan.state_reg[-1][-1]
    past = np.zeros((len(c["t"]), T + 1), bool)
    for b in range(len(c["t"])):
        ft = c["t"][b] - plan.dt_arr[0] - c["t0"][b]
        for i in range(T + 1):
            ft = np.round(ft + plan.dt_arr[min(i, T - 1)], 3)
            past[b, i] = not ft < end
    return past


def test_the_recording_holds_what_it_is_there_for(rec):
    assert tuple(rec["tables"]) == twin.REF_TABLES and os.path.getsize(GOLDEN) <= 1 << 20
    assert rec["q0"].shape == (19,) and int(rec["q0_is_SOLO12_Q0"]) == int(np.array_equal(rec["q0"], problems.SOLO12_Q0)) == 0
    tables = {n: twin.unpack_table(rec, n) for n in twin.REF_TABLES}
    for n, p in tables.items():
        c = twin.ref_cases(rec, n)
        B = len(c["t"])
        assert 24 <= B < 40 and c["x"].shape == (B, 37) and c["ref"]["ik_tasks"].shape == (B, p.n_col + 1, 33), n
        assert np.array_equal(p.state_reg[0][3:19], rec["q0"][3:]), n      # the first phase regularises about the reference's initial posture
        mt = np.round(c["t"] - c["t0"], 9)
        for e in sorted({float(r[0][k]) for r in p.cnt_plan for k in (4, 5)}):      # every contact-phase boundary and +- 0.01
            assert {float(np.round(e + d, 9)) for d in (-0.01, 0.0, 0.01)} <= set(mt.tolist()), (n, e)
        assert np.any(mt > p.cnt_plan[-1][0][5]) and np.any(c["t0"] != 0) and np.any(mt < 0), n
        assert {0.4125, 0.2375} <= set(c["t"].tolist()), n
        nominal, placed = c["kind"] == twin.STATE_NOMINAL, c["kind"] == twin.STATE_PLACED
        assert nominal.sum() == 3 and np.all(c["x"][nominal, :19] == problems.SOLO12_Q0) and np.all(c["x"][nominal, 19:] == 0), n
        assert np.all(c["x"][c["kind"] == twin.STATE_PERTURBED] == twin.states()[1]), n
        moved = twin.states()[1].copy()
        moved[:3] += rec["q0"][:3] - problems.SOLO12_Q0[:3]
        assert c["t"][placed].tolist() == [0.05, 0.88, 1.5] and np.all(c["t0"][placed] == 0) and np.all(c["x"][placed] == moved), n
    # the features the synthetic hop table lacks
    assert tables["plan_jump"].dt_arr[0] == 1.2 / 30 and tables["plan_jump"].kp[0][0] == 0.0
    assert tables["plan_cartwheel"].swing_wt is None and len(tables["plan_cartwheel"].dt_arr) == tables["plan_cartwheel"].n_col + 1
    sw = tables["rearing"].swing_wt
    assert sw[0][2][0] == 0 and sw[0][1][5] != sw[0][0][5]      # a swing row of weight 0, and a window of foot 1 that is not foot 0's
    rj = tables["rearing_jump"]
    assert (len(rj.state_wt), len(rj.state_reg), len(rj.state_scale)) == (3, 2, 2) and not np.array_equal(rj.state_wt[1], rj.state_wt[2])
    assert all(p.ctrl_wt[0][0] == 0 and p.ctrl_scale[0][0] != 0 for p in tables.values())      # ctrl_wt[k][0] = 0 is the running weight
    assert tables["plan_cartwheel"].plan_freq[-1][-1] > tables["plan_cartwheel"].cnt_plan[-1][0][5]      # plan_freq past T


@pytest.mark.parametrize("name", twin.REF_TABLES)
def test_mirror_equals_the_recording_bit_for_bit(model, rec, name):
    c, got = mirror(model, rec, name)
    assert np.array_equal(got["X_nom"][:, 9:], c["ref"]["X_nom"][:, 9:])
    for k in twin.REF_OUTPUTS:
        if k != "X_nom":
            assert got[k].shape == c["ref"][k].shape and np.array_equal(got[k], c["ref"][k]), (name, k)
    gen = SoloAcyclicGen(model, model)
    gen._make_kd = lambda: twin._Kd(twin.unpack_table(rec, name).n_col)
    for b in (0, len(c["t"]) - 1):
        gen.update_motion_params(twin.unpack_table(rec, name), c["x"][b, :19], float(c["t0"][b]))
        assert gen.size == c["size"][b]
    # x_init is an input of the recording (oracle/rbd_np.py): the mirror's own kinematics (fk_np) agree with it to rounding
    assert np.allclose(got["x_init"], c["x_init"], rtol=0, atol=1e-12) and np.array_equal(c["ref"]["X_nom"][:, :9], c["x_init"])


def test_the_old_rule_fails_on_rearing_jump(model, rec):
    """Row len(state_reg) - 1 of state_wt past the end, the rule of the mirror before this recording, planted through the twin: it
    differs from the recording in state_w, at exactly the nodes past the state table's end, and in nothing else."""
    c, got = mirror(model, rec, "rearing_jump", fault="shared_last_row")
    past = past_the_state_end(rec, "rearing_jump")
    differs = np.any(got["state_w"] != c["ref"]["state_w"], axis=2)
    assert past.any() and not past.all() and np.array_equal(differs, past)
    assert np.any(past.any(axis=1) & ~past.all(axis=1))      # a case that reaches the end inside its horizon
    for k in twin.REF_OUTPUTS:
        if k not in ("state_w", "X_nom"):
            assert np.array_equal(got[k], c["ref"][k]), k
    for name in ("rearing", "plan_jump"):      # equally long lists: the planted rule is the reference's
        c, got = mirror(model, rec, name, fault="shared_last_row")
        assert np.array_equal(got["state_w"], c["ref"]["state_w"]), name


def test_where_the_centroidal_solve_of_rearing_can_be_compared(model, rec, oracle):
    """Why the GPU solve test takes the PLACED cases.  The twin's states stand at SOLO12_Q0, 0.2 m behind the tables' contact locations;
    there the reference's ADMM is in its chaotic regime from the first iteration on (tests/util.py: a CPU ensemble of the strict C
    oracle, the matrix-free one and 16 one-ulp perturbations of x_init of each) or turns non-finite, for every recorded case of
    `rearing` that starts in the first stance: two faithful implementations end 1e-3 apart, and the batch kernel and the single-problem
    handle are two.  With the base where the reference starts, the three cases of the solve test stay calm for all 10 iterations."""
    from tests.util import chaos_ensemble
    plan, c = twin.unpack_table(rec, "rearing"), twin.ref_cases(rec, "rearing")
    first_stance = (c["kind"] == twin.STATE_PERTURBED) & (c["t"] - c["t0"] >= 0) & (c["t"] - c["t0"] < plan.cnt_plan[0][0][5])
    pick = np.flatnonzero(first_stance | (c["kind"] == twin.STATE_PLACED))
    a = twin.plan_batch_np(model, plan, c["x"][pick], c["t"][pick], c["t0"][pick])
    H, B = plan.n_col, len(pick)
    b = problems.Batch("rearing", B, H, 4, model.total_mass, float(plan.rho), a["cnt_plan"], a["dt"], a["x_init"], a["X_nom"], a["X_ter"],
                       np.tile(plan.W_X, H)[None], np.asarray(plan.W_X_ter)[None], np.tile(plan.W_F, H)[None], a["bounds"], None, None, 1.0, {})
    with np.errstate(invalid="ignore"):
        _, ens = chaos_ensemble(b, pick, 10, oracle)
    placed = c["kind"][pick] == twin.STATE_PLACED
    print("first-stance cases at the twin's state: k_calm", ens["k_calm"][~placed].tolist(), "spread", ens["spread"][~placed].tolist())
    print("placed cases: k_calm", ens["k_calm"][placed].tolist(), "spread", ens["spread"][placed].tolist())
    assert (~placed).sum() >= 10 and np.all(ens["k_calm"][~placed] <= 1) and not np.any(ens["spread"][~placed] < 1e-5)      # (NaN: non-finite)
    assert placed.sum() == 3 and np.all(ens["k_calm"][placed] == 10) and np.all(ens["spread"][placed] < 1e-12)


@pytest.mark.parametrize("name", ("plan_jump", "rearing"))
def test_plan_freq_and_gains_equal_the_recording(model, rec, name):
    gen = SoloAcyclicGen(model, model)
    gen._make_kd = lambda: twin._Kd(1)
    gen.update_motion_params(twin.unpack_table(rec, name), rec["q0"], float(rec[name + "__grid_t0"]))
    grid, nan = rec[name + "__grid"], lambda v: np.nan if v is None else float(v)      # noqa: E731
    assert len(grid) == 30 and grid[0] < gen.t0 and grid[-1] - gen.t0 > gen.params.cnt_plan[-1][0][5]
    freq = np.array([nan(gen.get_plan_freq(float(t))) for t in grid])
    gains = np.array([[nan(v) for v in (gen.get_gains(float(t)) or (None, None))] for t in grid])
    assert np.array_equal(freq, rec[name + "__freq"], equal_nan=True) and np.array_equal(gains, rec[name + "__gains"], equal_nan=True)
    assert np.isnan(freq[0]) and np.array_equal(np.isnan(freq), grid - gen.t0 < 0)      # None before the motion's start, a row after it
    assert len(np.unique(rec["plan_jump__freq"][~np.isnan(freq)])) == 2 and len(np.unique(rec["plan_jump__gains"][~np.isnan(freq), 0])) == 2


def test_stand_raises_in_the_mirror_as_in_the_reference(model, rec):
    assert int(rec["stand_raised"]) == 1 and str(rec["stand_error"]) == "TypeError"
    plan = twin.hop_plan()
    plan.plan_freq = None      # what `stand` lacks
    gen = SoloAcyclicGen(model, model)
    gen._make_kd = lambda: twin._Kd(plan.n_col)
    with pytest.raises(TypeError):
        gen.update_motion_params(plan, problems.SOLO12_Q0, 0.0)


@pytest.mark.parametrize("name", twin.REF_TABLES)
def test_hold_np_equals_the_references_expansion(rec, name):
    g = lambda k: rec["%s__hold_%s" % (name, k)]      # noqa: E731
    T = twin.unpack_table(rec, name).n_col
    for j in range(2):
        dt = g("dt")[j]
        assert dt.shape == (T + 1,) and dt[T] == 0 and np.array_equal(dt[:T], twin.unpack_table(rec, name).dt_arr[:T])
        assert np.array_equal(twin.hold_np(g("xs")[j], dt, T + 1), g("xs_int")[j])
        assert np.array_equal(twin.hold_np(g("us")[j], dt, T), g("us_int")[j]) and np.array_equal(twin.hold_np(g("F")[j], dt, T), g("f_int")[j])
        assert len(g("xs_int")[j]) == len(g("us_int")[j]) == len(g("f_int")[j]) == sum(int(v / 0.001) for v in dt[:T])
    assert not np.array_equal(g("xs")[0], g("xs")[1])


def test_hold_edge_intervals(rec):
    for k in twin.HOLD_EDGES_MS:
        assert int((k / 1000) / 0.001) == k - 1 and round((k / 1000) / 0.001) == k, k
    knots, dt = twin.hold_edge_problems()
    assert np.array_equal(knots, rec["hold_edge_knots"]) and np.array_equal(dt, rec["hold_edge_dt"]) and len(dt) <= 9 and knots.shape[1:] == (13, 37)
    edges = [k / 1000 for k in twin.HOLD_EDGES_MS]
    assert [dt[b, 0] for b in range(6)] == edges and dt[6, 3:9].tolist() == edges and np.all(dt[7] == 0.04)
    for b in range(len(dt)):
        full = twin.hold_np(knots[b], dt[b], 12)
        n = int(rec["hold_edge_rows"][b])
        assert n == len(full) and np.array_equal(rec["hold_edge_out"][b, :n], full) and np.all(rec["hold_edge_out"][b, n:] == 0)
    assert rec["hold_edge_rows"].tolist() == [549 + k for k in twin.HOLD_EDGES_MS] + [600 - 6 * 50 + sum(twin.HOLD_EDGES_MS) - 6, 480]


# ---- the host packing of the device path (acyclic_batch.host_tables), walked as csrc/acyclic_plan.hip walks it ------------------------

def _table_row(tab, lo, hi, end, ft, past):
    """table_row of csrc/acyclic_plan.hip"""
    if ft < end:
        for k in range(len(tab)):
            if tab[k, lo] <= ft < tab[k, hi]:
                return k
        return -1
    return past


@pytest.mark.parametrize("name", twin.REF_TABLES)
def test_packed_rows_walked_as_the_kernel_walks_them_equal_the_recording(model, rec, name):
    """one row index per group on the packed tables gives what the reference's per-list rule gives: state_w, x_reg, ctrl_w and the
    two weights of every node of every recorded case (and of a NaN and two infinite times, against the mirror's rule)"""
    from bunmpc_amd.acyclic_batch import host_tables
    plan, c = twin.unpack_table(rec, name), twin.ref_cases(rec, name)
    h, state_end = host_tables(plan, model.nq, model.nv)
    T, ref = plan.n_col, c["ref"]
    ns, nc = len(h["tab_state_scale"]), len(h["tab_ctrl_scale"])
    assert ns == len(plan.state_reg) + 1 == len(h["tab_state_wt"]) == len(h["tab_state_reg"]) and nc == len(plan.ctrl_scale) + 1 == len(h["tab_ctrl_wt"])
    assert h["dt_arr"].shape == (T,) and state_end == plan.state_reg[-1][-1] and ("tab_swing_wt" in h) == (plan.swing_wt is not None)

    def rows(ft):
        return (_table_row(h["tab_state_scale"], 1, 2, state_end, ft, ns - 1), _table_row(h["tab_ctrl_scale"], 1, 2, h["tab_ctrl_scale"][nc - 1, 2], ft, nc - 1))

    neutral = np.zeros(37)
    neutral[6] = 1.0
    for b in range(len(c["t"])):
        ft = c["t"][b] - h["dt_arr"][0] - c["t0"][b]
        for i in range(T + 1):
            ft = np.round(ft + h["dt_arr"][min(i, T - 1)], 3)
            ks, kq = rows(ft)
            assert np.array_equal(ref["state_w"][b, i], h["tab_state_wt"][ks] if ks >= 0 else np.zeros(36)), (b, i)
            assert np.array_equal(ref["x_reg"][b, i], h["tab_state_reg"][ks] if ks >= 0 else neutral), (b, i)
            assert ref["ik_tasks"][b, i, 31] == (h["tab_state_scale"][ks, 0] if ks >= 0 else 0.0), (b, i)
            if i < T:
                assert np.array_equal(ref["ctrl_w"][b, i], h["tab_ctrl_wt"][kq] if kq >= 0 else np.zeros(18)), (b, i)
                assert ref["ik_tasks"][b, i, 32] == (h["tab_ctrl_wt"][kq, 0] if kq >= 0 else 0.0), (b, i)
            else:
                assert ref["ik_tasks"][b, i, 32] == (h["tab_ctrl_scale"][kq, 0] if kq >= 0 else 0.0), (b, i)
    assert rows(np.nan) == (ns - 1, nc - 1) == rows(np.inf) and rows(-np.inf) == (-1, -1)      # NaN fails ft < end: each list's last row


def test_a_window_that_outlasts_the_last_rows_end_is_cut_there(model):
    """a first control row whose window ends after the LAST row's: past the last row's end the reference takes the last row"""
    from bunmpc_amd.acyclic_batch import host_tables
    plan = twin.hop_plan()
    plan.ctrl_scale = [[1e-4, 0.0, 2.0], [3e-4, 0.5, 0.9]]
    h, _ = host_tables(plan, model.nq, model.nv)
    assert h["tab_ctrl_scale"][:, 1:].tolist() == [[0.0, 0.9], [0.5, 0.9], [0.9, np.inf]] and np.array_equal(h["tab_ctrl_wt"][2], plan.ctrl_wt[1][:18])
    a = twin.plan_np(model, plan, twin.states()[0], 0.6, 0.0)      # knots at 0.6 .. 1.15, the terminal node at 1.2
    tab = h["tab_ctrl_scale"]
    for i in range(13):
        ft = np.round(0.6 + 0.05 * i, 3)
        kq = _table_row(tab, 1, 2, tab[2, 2], ft, 2)
        assert kq == (0 if ft < 0.9 else 2) and a["ik_tasks"][i, 32] == (h["tab_ctrl_wt"][kq, 0] if i < 12 else tab[kq, 0]), i


@pytest.mark.parametrize("change,word", [(dict(state_wt=[]), "state_wt"), (dict(ctrl_scale=[]), "ctrl_scale"), (dict(state_reg=[np.zeros(38)]), "state_reg"),
                                         (dict(ctrl_wt=[np.zeros(19)]), "ctrl_wt"), (dict(state_scale="one"), "state_scale"), (dict(state_wt="one"), "state_wt"),
                                         (dict(state_reg=16), "state_reg"), (dict(ctrl_scale=16), "ctrl_scale"), (dict(swing_wt=[np.zeros((4, 5))]), "swing_wt"),
                                         (dict(dt_arr=np.full(11, 0.05)), "dt_arr")])
def test_a_malformed_table_is_refused_with_the_field_named(model, change, word):
    from bunmpc_amd.acyclic_batch import host_tables
    plan = twin.hop_plan()
    for k, v in change.items():
        if isinstance(v, str):      # "one": fewer rows than state_reg has
            v = getattr(plan, k)[:1]
        elif isinstance(v, int):      # more rows than the device's phase limit leaves room for
            v = [getattr(plan, k)[0]] * v
        setattr(plan, k, v)
    with pytest.raises(ValueError, match=word):
        host_tables(plan, model.nq, model.nv)


def _reference_dir():
    for d in (os.environ.get("BUNMPC_REFERENCE"), os.path.join(os.path.dirname(ROOT), "reference")):
        if d and os.path.isfile(os.path.join(d, "iterative_supervised_learning", "examples", "mpc", "abstract_acyclic_gen.py")):
            return d
    return None


def test_the_generator_reproduces_the_committed_file(rec):
    """the one test that looks for the reference (beside the repository, or where BUNMPC_REFERENCE points)"""
    ref = _reference_dir()
    if ref is None:
        pytest.skip("the reference is not on this machine")
    spec = importlib.util.spec_from_file_location("make_golden_acyclic", GENERATOR)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out, _ = gen.record(ref)
    assert sorted(out) == sorted(rec)
    for k, v in out.items():
        v = np.asarray(v)
        assert v.dtype == rec[k].dtype and v.shape == rec[k].shape, k
        assert np.array_equal(v, rec[k], equal_nan=v.dtype.kind == "f"), k
