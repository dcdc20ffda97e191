"""include/ext/bunmpc_dataset.h on the GPU, through bunmpc_amd/dataset_device.py::DeviceDatabase and the C-ABI: the ring bit for bit
against the twin (tests/dataset_np.py) after every step of sequences that are enqueued on one stream and read back once, the
statistics against exact arithmetic, the batch view against numpy's (v - mean) / std, the generator's dict, and the way to the host
class and back."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import dataset_np as twin

pytestmark = pytest.mark.gpu

ROBOTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bunmpc_amd", "robots")
DEV = "cuda:0"


def _groups(rng, shape, w_cc=12):
    g = dict(states=rng.normal(size=shape + (43,)), actions=rng.normal(size=shape + (12,)), vc_goals=rng.normal(size=shape + (5,)))
    if w_cc:
        g["cc_goals"] = rng.normal(size=shape + (w_cc,))
    return g


def _dev(a, dtype=None):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _off_by_one_element(a):
    """the array as a device tensor that starts 8 bytes into its allocation: only 8-byte aligned"""
    import torch
    flat = torch.empty(a.size + 1, dtype=torch.float64, device=DEV)
    flat[1:].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    view = flat[1:].view(a.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    return view


def run_sequence(limit, steps, goal_horizon=1, unaligned=()):
    """steps: [dict(arrays..., rows=, keep=, drop_nonfinite=)]; every step is appended to a DeviceDatabase and to the twin, the device
    buffers and header are cloned on the stream after every step, and everything is read back at the end: equal bit for bit"""
    import torch
    from bunmpc_amd.dataset_device import DeviceDatabase
    w_cc = 12 * goal_horizon
    db, tw = DeviceDatabase(limit, goal_horizon=goal_horizon, device=DEV, max_problems=4096), twin.TwinDatabase(limit, w_cc=w_cc)
    snaps, want = [], []
    for i, step in enumerate(steps):
        opts = {k: step[k] for k in ("rows", "keep", "drop_nonfinite") if k in step}
        arrays = {k: v for k, v in step.items() if k in twin.GROUPS}
        n = tw.append(**arrays, **opts)
        want.append(({k: v.copy() for k, v in tw.buf.items()}, (tw.start, tw.length, n)))
        to_dev = _off_by_one_element if i in unaligned else _dev
        dev_opts = dict(opts)
        for k in ("rows", "keep"):
            if k in dev_opts:
                dev_opts[k] = _dev(np.asarray(dev_opts[k]), torch.int32)
        db.append(**{k: to_dev(v) for k, v in arrays.items()}, **dev_opts)
        snaps.append(({k: getattr(db, k).clone() for k in twin.GROUPS}, db.header.clone()))
    for i, ((bufs, header), (wbufs, whead)) in enumerate(zip(snaps, want)):
        assert tuple(header.cpu().numpy()[:3]) == whead, (i, header.cpu().numpy(), whead)
        for k in twin.GROUPS:
            got = bufs[k].cpu().numpy()
            assert np.array_equal(got, wbufs[k], equal_nan=True), (i, k, np.argwhere(got != wbufs[k])[:4])
    return db, tw


# ---- the ring -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("limit", [50, 51])
def test_ring_of_flat_appends(limit):
    """(n, w) appends; limit = 51: 51 * 43 and 51 * 5 are odd, so pairs of elements straddle the ring's end in both groups once it wraps"""
    rng = np.random.default_rng(0)
    run_sequence(limit, [_groups(rng, (n,)) for n in (7, 30, 20, 0, 49, 50, 120, 3)], unaligned=(1, 4))


@pytest.mark.parametrize("goal_horizon", [1, 3])
def test_ring_of_problem_appends_with_rows_and_keep(goal_horizon):
    """limit = 997 (odd: the ring's end falls inside an element pair of the 43-wide and 5-wide groups), (B, R) = (70, 50) and, for the
    pairs inside a problem's block, (33, 7): rows[b] drawn from 0..R with several 0 and R, keep drops a fifth, one append with every
    problem dropped, one whose kept rows exceed limit"""
    rng = np.random.default_rng(1)
    steps = []
    for i in range(6):
        B, R = (70, 50) if i % 2 == 0 else (33, 7)
        g = _groups(rng, (B, R), 12 * goal_horizon)
        rows = rng.integers(0, R + 1, size=B)
        rows[rng.choice(B, 6, replace=False)] = 0
        rows[rng.choice(B, 6, replace=False)] = R
        rows[0] = R + 5                                   # clipped to R
        rows[1] = -3                                      # clipped to 0
        keep = (rng.random(B) > 0.2).astype(np.int32)
        if i == 3:
            keep[:] = 0                                   # nothing goes in
        if i == 4:
            rows[:], keep[:] = R, 1                       # 3500 rows into 997 slots
        g.update(rows=rows, keep=keep)
        steps.append(g)
    steps.append(_groups(rng, (40, 50), 12 * goal_horizon))       # no rows, no keep: 2000 rows, again more than the ring holds
    db, tw = run_sequence(997, steps, goal_horizon=goal_horizon, unaligned=(2,))
    assert tw.length == 997 and tw.start != 0 and len(db) == 997 and db.start == tw.start


def test_ring_across_the_prefix_chunks():
    """B = 2500 problems of R = 3 rows: the prefix works in chunks of 1024 problems, so two of its seams lie inside the batch; R w is
    odd for the 43-wide and 5-wide groups, so every other problem's block starts 8 bytes off a 16-byte boundary"""
    rng = np.random.default_rng(2)
    steps = []
    for i in range(2):
        g = _groups(rng, (2500, 3))
        g.update(rows=rng.integers(0, 4, size=2500), keep=(rng.random(2500) > 0.2).astype(np.int32))
        steps.append(g)
    run_sequence(4099, steps)


def test_ring_without_the_cc_group_and_without_vc_goals():
    import torch
    from bunmpc_amd.dataset_device import DeviceDatabase
    rng = np.random.default_rng(3)
    run_sequence(51, [_groups(rng, (n,), 0) for n in (40, 30, 60)], goal_horizon=0)
    steps = [_groups(rng, (n,)) for n in (40, 30, 25, 20)]
    del steps[1]["vc_goals"], steps[3]["vc_goals"], steps[2]["cc_goals"]
    db, tw = run_sequence(51, steps)
    # slot 5 was written by the second and the last append, neither of which brought vc_goals: it holds those of the first
    assert np.array_equal(tw.buf["vc_goals"][5], steps[0]["vc_goals"][5]) and np.array_equal(tw.buf["states"][5], steps[3]["states"][12])
    s = torch.zeros((2, 43), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        db.append(s, s[:, :12].contiguous())
    with pytest.raises(RuntimeError, match="without that group"):
        DeviceDatabase(10, goal_horizon=0, device=DEV).append(s, s[:, :12].contiguous(), cc_goals=s[:, :12].contiguous())


def test_drop_nonfinite():
    rng = np.random.default_rng(4)
    g = _groups(rng, (9, 6))
    rows = np.array([6, 4, 6, 3, 6, 0, 6, 5, 6])
    g["actions"][0, 5, 11] = np.nan          # the last kept row of problem 0
    g["cc_goals"][1, 2, 0] = -np.inf         # problem 1
    g["states"][3, 4, 7] = np.nan            # beyond rows[3]: problem 3 stays
    g["vc_goals"][7, 4, 4] = np.inf          # the last element of problem 7's kept rows
    on = dict(g, rows=rows, drop_nonfinite=True)
    off = dict(g, rows=rows, drop_nonfinite=False)
    _, tw = run_sequence(200, [on, off, dict(g, drop_nonfinite=True)])
    assert tw.length == (6 + 3 + 6 + 6 + 6) + rows.sum() + 6 * 5


# ---- the generator's dict -----------------------------------------------------------------------------------------------------------------

def test_append_step():
    import torch
    from bunmpc_amd import dataset, problems, urdf_model
    from bunmpc_amd.datagen import PlanLabelGenerator
    from bunmpc_amd.dataset_device import DeviceDatabase
    model = urdf_model.RobotModel.from_json(open(os.path.join(ROBOTS, "solo12.json")).read())
    B = 6
    wb = problems.make_wb_batch(model, B)
    q, v = torch.as_tensor(wb.x[:, :19], device=DEV), torch.as_tensor(wb.x[:, 19:], device=DEV)
    t0 = torch.as_tensor(np.array([0.0, 0.05, 0.1, 0.0, 0.05, 0.1]), device=DEV)
    vd = torch.as_tensor(wb.dyn.meta["v_des_body"], device=DEV)
    out = PlanLabelGenerator(model, goal_horizon=1, device=DEV).step(q, v, t0, vd, perturb=False, episode_length=200)
    R = out["states"].shape[1]
    host = {k: out[k].cpu().numpy() for k in ("states", "actions", "vc_goals", "cc_goals")}
    rows, status = out["goal_rows"].cpu().numpy(), out["goal_status"].cpu().numpy()
    assert R == 50 and np.all(status == 0)

    def old_way(problems_in):
        db = dataset.Database(1000)
        sel = [(b, r) for b in problems_in for r in range(rows[b])]
        db.append(*(np.array([host[k][b, r] for b, r in sel]) for k in ("states", "actions")),
                  vc_goals=np.array([host["vc_goals"][b, r] for b, r in sel]), cc_goals=np.array([host["cc_goals"][b, r] for b, r in sel]))
        return db.arrays()

    def same(dev_db, arrs):
        got = dev_db.to_host().arrays()
        return set(got) == set(arrs) and all(np.array_equal(got[k], arrs[k]) for k in arrs)

    assert same(DeviceDatabase(1000, device=DEV).append_step(out), old_way(range(B)))
    forced = dict(out, goal_status=out["goal_status"].clone())
    forced["goal_status"][2] = 4
    assert same(DeviceDatabase(1000, device=DEV).append_step(forced), old_way([0, 1, 3, 4, 5]))
    forced["rejected"] = torch.tensor([4], device=DEV)
    assert same(DeviceDatabase(1000, device=DEV).append_step(forced, drop_rejected=True), old_way([0, 1, 3, 5]))
    assert same(DeviceDatabase(1000, device=DEV).append_step(forced), old_way([0, 1, 3, 4, 5]))
    # a data set without the cc group takes the states, actions and vc_goals of every problem
    plain = DeviceDatabase(1000, goal_horizon=0, device=DEV).append_step(out).to_host()
    assert plain.length == B * R and np.array_equal(plain.vc_goals[:B * R], host["vc_goals"].reshape(B * R, 5))


# ---- moments ----------------------------------------------------------------------------------------------------------------------------

def _moment_data(rng, n):
    from tests.test_dataset_device_cpu import moment_data
    return moment_data(rng, n)


def _moments(db):
    db.calc_input_mean_std()
    return [t.cpu().numpy() for t in (db.states_mean, db.states_std, db.cc_goals_mean, db.cc_goals_std)]


def test_moments_against_exact_arithmetic():
    """A ring of limit = 2000 that has wrapped (two workgroups of partial sums), and length = 1 and 3: mean and std within twice the
    bounds of tests/dataset_np.py::moment_violations of the exact values -- one bound for the device's order of summation, one for
    the reference's.  The device rounds where numpy does (the subtraction, the square, every addition, the division, the square
    root), in a tree of another shape; no operation is fused.  A second call returns the same bits; an empty data set gives NaN."""
    from bunmpc_amd.dataset_device import DeviceDatabase
    rng = np.random.default_rng(5)
    db = DeviceDatabase(2000, device=DEV)
    assert all(np.all(np.isnan(a)) for a in _moments(db))
    tw = twin.TwinDatabase(2000)
    for n in (1, 2, 1500, 900):
        s, c = _moment_data(rng, n)
        a = rng.normal(size=(n, 12))
        db.append(_dev(s), _dev(a), cc_goals=_dev(c))
        tw.append(s, a, cc_goals=c)
        if n == 2 or n == 900:
            got, again = _moments(db), _moments(db)
            assert all(np.array_equal(g, h) for g, h in zip(got, again))
            assert tw.length == (3 if n == 2 else 2000)
            for k, (mean, std) in (("states", got[0:2]), ("cc_goals", got[2:4])):
                assert twin.moment_violations(mean, std, twin.exact_moments(tw.buf[k][:tw.length]), tw.length, factor=2) == [], k
    one = DeviceDatabase(7, device=DEV)
    s, c = _moment_data(rng, 1)
    one.append(_dev(s), _dev(s[:, :12]), cc_goals=_dev(c))
    got = _moments(one)
    assert np.array_equal(got[0], s[0]) and np.all(got[1] == 0) and np.array_equal(got[2], c[0]) and np.all(got[3] == 0)
    assert one.get_database_mean_std()[2] is one.cc_goals_mean
    one.set_goal_type("vc")
    assert one.get_database_mean_std()[2:] == [0.0, 1.0]
    one.set_normalize_input(False)
    assert one.get_database_mean_std() is None


def test_moments_through_the_c_abi_without_the_cc_group():
    import torch
    from bunmpc_amd import _lib, _lib_dataset
    from bunmpc_amd.dataset_device import DeviceDatabase
    rng = np.random.default_rng(6)
    db = DeviceDatabase(1500, goal_horizon=0, device=DEV)
    s, _ = _moment_data(rng, 1100)
    db.append(_dev(s), _dev(s[:, :12]), vc_goals=_dev(s[:, :5]))
    mean, std = torch.empty(43, dtype=torch.float64, device=DEV), torch.empty(43, dtype=torch.float64, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(_lib_dataset.lib().bmpc_dataset_moments_device(C.byref(db.desc), mean.data_ptr(), std.data_ptr(), None, None, stream))
    assert twin.moment_violations(mean.cpu().numpy(), std.cpu().numpy(), twin.exact_moments(s), 1100, factor=2) == []


# ---- batch ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 64, 1000])
def test_batch(n):
    """x, y equal numpy's (v - mean) / std with the device's own statistics read back, and the raw rows; both goal types, both settings
    of normalise, repeated indices, -1 and length (rows of NaN), the constant column (std == 0: what IEEE gives)"""
    from bunmpc_amd.dataset_device import DeviceDatabase
    rng = np.random.default_rng(7)
    db, tw = DeviceDatabase(300, device=DEV), twin.TwinDatabase(300)
    for m in (200, 50):
        s, c = _moment_data(rng, m)
        a, g = rng.normal(size=(m, 12)), rng.normal(size=(m, 5))
        db.append(_dev(s), _dev(a), vc_goals=_dev(g), cc_goals=_dev(c))
        tw.append(s, a, vc_goals=g, cc_goals=c)
    got = _moments(db)
    stats = dict(states=(got[0], got[1]), cc_goals=(got[2], got[3]))
    assert got[1][5] <= 2 * 250 * 2.0 ** -53 * 0.1         # the constant column: its std is 0 or a few ulps of 0.1, and x takes what IEEE gives
    index = rng.integers(0, 250, size=n)
    index[: n // 4] = index[n // 2: n // 2 + n // 4]      # repeated rows
    if n > 1:
        index[n // 3], index[-1] = -1, 250
    for goal_type in ("vc", "cc"):
        for normalise in (True, False):
            db.set_goal_type(goal_type)
            db.set_normalize_input(normalise)
            x, y = db.batch(_dev(index))
            wx, wy = tw.batch(index, goal_type, normalise, stats)
            assert x.shape == wx.shape and y.shape == wy.shape
            assert np.array_equal(x.cpu().numpy(), wx, equal_nan=True) and np.array_equal(y.cpu().numpy(), wy, equal_nan=True), (goal_type, normalise)
            if n > 1:
                assert np.all(np.isnan(wx[-1])) and np.all(np.isnan(wy[n // 3])) and np.all(np.isfinite(wy[0]))
    x, y = db.batch(_dev(np.zeros(0, dtype=np.int64)))
    assert x.shape == (0, 55) and y.shape == (0, 12)


# ---- to the host class and back -----------------------------------------------------------------------------------------------------------

def test_round_trip_and_save(tmp_path):
    from bunmpc_amd.dataset_device import DeviceDatabase
    rng = np.random.default_rng(8)
    db = DeviceDatabase(60, goal_horizon=3, device=DEV)
    for n in (45, 40):
        db.append(**{k: _dev(v) for k, v in _groups(rng, (n,), 36).items()})
    host = db.to_host()
    assert (host.start, host.length, host.limit) == (25, 60, 60) and host.cc_goals.shape == (60, 36)
    back = DeviceDatabase.from_host(host, device=DEV)
    again = back.to_host()
    assert (again.start, again.length) == (host.start, host.length) and back.goal_horizon == 3
    assert all(np.array_equal(getattr(again, k), getattr(host, k)) for k in twin.GROUPS)
    extra = _groups(rng, (7,), 36)                        # the two go on alike
    back.append(**{k: _dev(v) for k, v in extra.items()})
    host.append(**extra)
    assert back.start == host.start and all(np.array_equal(getattr(back.to_host(), k), getattr(host, k)) for k in twin.GROUPS)
    a, b = back.save(str(tmp_path / "dev"), 2, config={"n": 1}), host.save(str(tmp_path / "host"), 2, config={"n": 1})
    assert os.path.basename(a) == os.path.basename(b)
    assert open(a, "rb").read() == open(b, "rb").read() and (tmp_path / "dev" / "config.pkl").exists()
    assert set(back.arrays()) == {"states", "vc_goals", "cc_goals", "actions"}
