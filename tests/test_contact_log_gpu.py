"""include/ext/bunmpc_contact_log.h on the GPU, through bunmpc_amd/contact_log.py::DeviceContactLog: every output of
bmpc_contact_log_goals_device bit for bit against the host twin (contact_log.host_batch, which tests/test_contact_log_cpu.py ties to the
reference's recorded outputs), the failed-state test, the other groups of logged episodes (episode_groups) and the way into the device
data set (DeviceDatabase.append_episodes).  Small shapes: the seams of the events kernel's 64-row blocks and of its 256-row chunks are crossed."""
import os

import numpy as np
import pytest

from bunmpc_amd import contact_log
from tests import contact_log_cases as cases

pytestmark = pytest.mark.gpu

ROBOTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bunmpc_amd", "robots")
DEV = "cuda:0"
OUTPUTS = ("schedule", "counts", "goals", "rows", "status", "failed_step")
STARTS = (0, 0, 7, 130, 370)


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _read(log):
    return {k: getattr(log, k).cpu().numpy() for k in OUTPUTS}


def _equal(got, tw, what):
    for k in OUTPUTS:
        assert got[k].shape == tw[k].shape and got[k].dtype == tw[k].dtype, (what, k, got[k].shape, tw[k].shape, got[k].dtype)
        assert np.array_equal(got[k], tw[k], equal_nan=True), (what, k, np.argwhere(~((got[k] == tw[k]) | (np.isnan(got[k]) & np.isnan(tw[k]))))[:4])


def _run(ee_pos, com, start, episode_length, goal_horizon, max_events, max_rows=None, twice=False):
    """the device call and the twin on one batch; with `twice`, two calls enqueued back to back into the same buffers"""
    import torch
    B, T = ee_pos.shape[:2]
    log = contact_log.DeviceContactLog(B, T, goal_horizon=goal_horizon, max_events=max_events, max_rows=max_rows, device=DEV)
    args = (_dev(ee_pos), _dev(com), _dev(np.asarray(start), torch.int32), episode_length)
    log.build(*args)
    first = {k: getattr(log, k).clone() for k in OUTPUTS} if twice else None
    if twice:
        log.build(*args)
    got = _read(log)
    if twice:
        for k in OUTPUTS:
            assert np.array_equal(first[k].cpu().numpy(), got[k], equal_nan=True), k
    tw = contact_log.host_batch(ee_pos, com, start, episode_length, goal_horizon=goal_horizon, max_events=max_events, max_rows=max_rows)
    return got, tw


def seam_rows(T):
    """rising edges exactly at rows 0, 63, 64, 127 and 128, and at 255, 256 and 257 about the seam of the events kernel's 256-row chunks
    (those below T); two feet landing at rows 64, 128 and 256"""
    rows = [[0, 64, 128, 256], [63, 127, 255], [64, 257], [128, 250, 256]]
    return [[r for r in foot if r < T] for foot in rows]


def seam_log(T, start):
    """... and foot 2 standing from row 240 through row 256 to row 270, but for a NaN x at row 255: neither an edge across the chunk seam
    (the carried bit says not cleared) nor at row 257, which the list above names"""
    rows = seam_rows(T)
    ee, com = cases.edges_log(T, [rows[0], rows[1], [r for r in rows[2] if r != 257], rows[3]], start)
    if T > 270:
        ee[240:271, 2] = [0.31, 0.2, 1e-3]
        ee[255, 2, 0] = np.nan
    return ee, com


def episodes(T):
    """B = 5 episodes with the start steps STARTS: the seam log from step 0 (row 0 is step 0: skipped) and from step 7 (recorded), trot,
    bound and jump logs"""
    logs = [seam_log(T, 0), cases.synthetic_log("trot", T, 0, period=24), seam_log(T, 7),
            cases.synthetic_log("bound", T, 130, period=30), cases.synthetic_log("jump", T, 370, period=20)]
    return np.stack([l[0] for l in logs]), np.stack([l[1] for l in logs])


@pytest.mark.parametrize("goal_horizon", [1, 3])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130, 200, 300])
def test_outputs_equal_the_twin_across_block_seams(T, goal_horizon):
    """episode_length = 400: the episode that starts at step 370 ends 30 rows into its log; max_rows below the rows at goal horizon 3"""
    ee_pos, com = episodes(T)
    max_rows = max(1, T // 3) if goal_horizon == 3 else None
    got, tw = _run(ee_pos, com, STARTS, 400, goal_horizon, max_events=64, max_rows=max_rows, twice=(T == 130))
    _equal(got, tw, (T, goal_horizon))
    if T >= 130:
        want = [3, 2, 1, 1] if T < 300 else [4, 3, 2, 3]                   # foot 2 at T = 300: rows 64 and 240 only
        assert tw["counts"][2].tolist() == want and tw["counts"][0].tolist() == [want[0] - 1] + want[1:]      # row 0 at step 0 is not recorded
        assert np.all(tw["status"] == 0) and np.all(tw["rows"][[1, 3]] > 0)
        assert tw["counts"][4].sum() > 0 and np.all(tw["schedule"][4, :, :, 0].max(axis=1) < 400)        # the log is longer than the episode
        if goal_horizon == 3:
            assert tw["rows"][1] == max_rows and contact_log.host_batch(ee_pos, com, STARTS, 400, goal_horizon=3, max_events=64)["rows"][1] > max_rows


def special_batch():
    """T = 130: [a foot without events from step 0, the same from step 7, one event in all, two events in all, the log whose goal horizon 5
    runs past the schedule, a trot log of more switches than max_events = 12, the NaN and threshold rows, a contact at x == 0.0]"""
    T = 130
    above = np.nextafter(1e-12, 1.0)
    logs = [cases.edges_log(T, [[3, 9, 100], [], [5, 70], [12, 90]], 0), cases.edges_log(T, [[3, 9, 100], [], [5, 70], [12, 90]], 7),
            cases.edges_log(T, [[], [17], [], []], 5), cases.edges_log(T, [[20], [], [31], []], 0),
            cases.edges_log(T, [[10, 20, 30, 40, 50, 60, 95], [90], [91], [92]], 0), cases.synthetic_log("trot", T, 0, period=24)]
    ee, com = cases.edges_log(T, [[100], [101], [102], [103]], 0)
    ee[2, 0, 0], ee[4, 0, 0], ee[6, 0, 0], ee[8, 0, 0] = 1e-12, above, -1e-12, -above
    ee[63, 1], ee[64, 1] = [np.nan, 0.1, 0.1], [0.2, 0.1, 0.0]          # a NaN x in the last row of a block: no cleared predecessor across the seam
    ee[70, 2], ee[71, 2] = [np.nan, 0.1, 0.1], [0.2, 0.1, 0.0]
    ee[80, 3] = [0.2, np.nan, 0.0]                                        # a NaN beside x goes into the event
    logs.append((ee, com))
    ee, com = cases.edges_log(T, [[100], [101], [102], [103]], 0)
    ee[20:25, 0] = [0.0, 0.4, 0.01]
    logs.append((ee, com))
    return np.stack([l[0] for l in logs]), np.stack([l[1] for l in logs]), (0, 7, 5, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("goal_horizon", [1, 3, 5])
def test_statuses_and_quirks_equal_the_twin(goal_horizon):
    ee_pos, com, start = special_batch()
    got, tw = _run(ee_pos, com, start, 135, goal_horizon, max_events=12)
    _equal(got, tw, goal_horizon)
    s = got["status"]
    assert (s[0], got["rows"][0]) == (0, 0) and s[1] == contact_log.START_AFTER_END           # end_time = 0
    assert s[2] == contact_log.FEW_SWITCHES and got["counts"][2].sum() == 1
    assert (s[3], got["rows"][3], got["counts"][3].sum()) == (0, 0, 2)                        # two feet without events: end_time = 0, no row to raise on
    assert (s[4], got["rows"][4]) == ((contact_log.PAST_SCHEDULE, 60) if goal_horizon == 5 else (0, 90))
    assert s[5] == contact_log.EVENTS_OVERFLOW and got["counts"][5].sum() > 12 and got["rows"][5] == 0
    assert got["counts"][6].tolist() == [3, 1, 1, 2] and np.isnan(got["schedule"][6, 3, 0, 2]) and got["schedule"][6, 0, :2, 0].tolist() == [4.0, 8.0]
    assert got["counts"][7].tolist() == [1, 1, 1, 1]
    for b in np.flatnonzero(s & (contact_log.FEW_SWITCHES | contact_log.START_AFTER_END | contact_log.EVENTS_OVERFLOW)):
        assert not got["goals"][b].any()


def test_no_episodes():
    import torch
    log = contact_log.DeviceContactLog(0, 50, device=DEV)
    log.build(torch.zeros((0, 50, 4, 3), dtype=torch.float64, device=DEV), torch.zeros((0, 50, 3), dtype=torch.float64, device=DEV),
              torch.zeros(0, dtype=torch.int32, device=DEV), 50)
    assert log.goals.shape == (0, 50, 12) and log.rows.shape == (0,)


# ---- failed states ----------------------------------------------------------------------------------------------------------------------

def failing_rows():
    """64 episodes of T = 40 as rows [q, v]: episode b has one row after the grace rows whose roll, pitch or height sits on one side of a
    threshold -- angles 1e-6 degrees and more from fail_angle = 30, heights on both sides of z_min = 0.1 and of 2.0 and exactly z_min --
    and, every fourth episode, a failing row within the grace rows as well (which does not count)"""
    rng = np.random.default_rng(7)
    B, T = 64, 40
    x = rng.normal(0, 0.3, size=(B, T, 37))
    x[:, :, 2] = 0.23 + 0.01 * rng.random((B, T))
    offsets = (1e-6, -1e-6, 1e-3, -1e-3, 5.0, -5.0)
    for b in range(B):
        for r in range(T):
            x[b, r, 3:7] = cases.quaternion_xyzw(rng.uniform(-25, 25), rng.uniform(-25, 25), rng.uniform(-180, 180))
        r, kind, off = 11 + (b * 7) % 29, b % 4, offsets[(b // 4) % 6]
        sign = 1.0 if (b // 24) % 2 == 0 else -1.0
        if kind == 0:
            x[b, r, 3:7] = cases.quaternion_xyzw(sign * (30.0 + off), rng.uniform(-20, 20), rng.uniform(-180, 180))
        elif kind == 1:
            x[b, r, 3:7] = cases.quaternion_xyzw(rng.uniform(-20, 20), sign * (30.0 + off), rng.uniform(-180, 180))
        elif kind == 2:
            x[b, r, 2] = (0.1, np.nextafter(0.1, 0.0), np.nextafter(0.1, 1.0), 0.0999, 0.05, 0.1)[(b // 4) % 6]
        else:
            x[b, r, 2] = (2.0, np.nextafter(2.0, 3.0), np.nextafter(2.0, 0.0), 2.5, 1.99, 2.0)[(b // 4) % 6]
        if b % 4 == 0:
            x[b, 10, 2] = 0.01
    return x


def test_failed_states_equal_the_twin():
    """failed_step against the twin's, the angles within 1e-12 degrees of it: about 35 ulp of 180 degrees for two library calls of a few
    ulp each and one multiply.  The observed maximum is printed."""
    import torch
    x = failing_rows()
    B, T = x.shape[:2]
    logs = [cases.synthetic_log("trot", T, 0, period=10) for _ in range(B)]
    ee_pos, com = np.stack([l[0] for l in logs]), np.stack([l[1] for l in logs])
    xd = _dev(x)
    log = contact_log.DeviceContactLog(B, T, max_events=40, want_angles=True, device=DEV)
    log.build(_dev(ee_pos), _dev(com), torch.zeros(B, dtype=torch.int32, device=DEV), T, q=xd[:, :, :19], z_min=0.1, fail_angle=30, gait_period=0.01)
    assert log.desc.s_q == 37 and log.desc.grace == 10.0      # the rows [q, v] in place
    got = _read(log)
    tw = contact_log.host_batch(ee_pos, com, np.zeros(B, int), T, max_events=40, q=x, z_min=0.1, fail_angle=30.0, grace=0.01 / 0.001)
    _equal(got, tw, "failed states")
    err = np.abs(log.angles.cpu().numpy() - tw["angles"]).max()
    print("largest angle difference to the twin: %.3g degrees" % err)
    assert err <= 1e-12
    failed = got["failed_step"] >= 0
    assert 20 <= failed.sum() <= 44 and np.all(got["failed_step"][failed] > 10)
    assert np.all(got["rows"][failed] == 0) and np.all(got["status"][failed] & contact_log.FAILED_STATE) and np.all(got["status"][~failed] == 0)
    assert np.all(got["rows"][~failed] > 0) and not got["goals"][failed].any()
    heights = [b for b in range(B) if b % 4 == 2 and (b // 4) % 6 in (0, 5)]      # exactly z_min: the comparison is strict
    assert heights and not failed[heights].any()
    # without q: the same goals, no failure
    log.build(_dev(ee_pos), _dev(com), torch.zeros(B, dtype=torch.int32, device=DEV), T)
    again = _read(log)
    assert np.all(again["failed_step"] == -1) and np.all(again["status"] == 0) and np.array_equal(again["goals"][~failed], got["goals"][~failed])


def test_first_failing_row_of_several_across_waves():
    """T = 200: an episode spans four waves of the failed-state kernel.  Failing rows 150, 70 and 75 (two waves, and two lanes of one
    wave): 70; rows 130 and 131 of one wave: 130; a failing row within the grace rows and one behind the episode's end only: none"""
    import torch
    B, T = 3, 200
    x = np.zeros((B, T, 37))
    x[:, :, 2], x[:, :, 6] = 0.23, 1.0
    for b, rows in enumerate(([150, 70, 75], [130, 131], [5, 190])):
        for k, r in enumerate(rows):
            if k % 2:
                x[b, r, 3:7] = cases.quaternion_xyzw(0.0, -35.0, 20.0)
            else:
                x[b, r, 2] = 0.01
    logs = [cases.synthetic_log("trot", T, 0, period=24) for _ in range(B)]
    ee_pos, com = np.stack([l[0] for l in logs]), np.stack([l[1] for l in logs])
    log = contact_log.DeviceContactLog(B, T, max_events=64, device=DEV)
    log.build(_dev(ee_pos), _dev(com), torch.zeros(B, dtype=torch.int32, device=DEV), 180, q=_dev(x)[:, :, :19], gait_period=0.01)
    got = _read(log)
    tw = contact_log.host_batch(ee_pos, com, np.zeros(B, int), 180, max_events=64, q=x, z_min=0.1, fail_angle=30.0, grace=0.01 / 0.001)
    _equal(got, tw, "several failing rows")
    assert got["failed_step"].tolist() == [70, 130, -1] and got["status"].tolist() == [contact_log.FAILED_STATE, contact_log.FAILED_STATE, 0]
    assert got["rows"][2] > 0 and not got["goals"][:2].any()


# ---- the other groups and the data set ---------------------------------------------------------------------------------------------------

def test_episode_groups_against_the_numpy_kinematics():
    """states and com within 1e-11 of fk_np relative to max(1, the row's largest entry), the bound of tests/test_id_gpu.py; the phase
    column bit for bit"""
    import torch
    from bunmpc_amd import fk_np, problems, urdf_model
    from oracle import rbd_np
    model = urdf_model.RobotModel.from_json(open(os.path.join(ROBOTS, "solo12.json")).read())
    feet = ["FL_FOOT", "FR_FOOT", "HL_FOOT", "HR_FOOT"]
    rng = np.random.default_rng(3)
    B, T = 3, 33
    q, v = np.zeros((B, T, 19)), rng.normal(0, 1.0, (B, T, 18))
    for b in range(B):
        for r in range(T):
            base = rbd_np.neutral(model)
            base[:3] = rng.normal(0, 0.5, 3)
            q[b, r] = rbd_np.integrate(model, base, rng.normal(0, 0.6, 18))
    start, v_des, w_des = np.array([0, 7, 2990]), rng.normal(0, 0.3, (B, 3)), rng.normal(0, 0.2, B)
    gait = problems.TROT
    x = _dev(np.concatenate([q, v], axis=2))
    for qd, vd in ((x[:, :, :19], x[:, :, 19:]), (_dev(q), _dev(v))):      # rows [q, v] in place, and separate arrays
        states, vc, com = contact_log.episode_groups(model, feet, qd, vd, _dev(start, torch.int32), _dev(v_des), _dev(w_des), gait)
        kin = fk_np.kinematics(model, q.reshape(-1, 19))
        foot = fk_np.frame_positions(model, kin, feet)
        ref = np.concatenate([v.reshape(-1, 18), (q.reshape(-1, 19)[:, None, 0:2] - foot[:, :, 0:2]).reshape(-1, 8), q.reshape(-1, 19)[:, 2:]], axis=1)
        for got, want in ((states.cpu().numpy().reshape(-1, 43), ref), (com.cpu().numpy().reshape(-1, 3), kin["com"])):
            scale = np.maximum(1.0, np.abs(want).max(axis=1, keepdims=True))
            assert got.shape == want.shape and (np.abs(got - want) / scale).max() < 1e-11, (np.abs(got - want) / scale).max()
        o = start[:, None] + np.arange(T)[None, :]
        vc = vc.cpu().numpy()
        assert np.array_equal(vc[:, :, 0], ((o * 0.001) % gait.gait_period) / gait.gait_period)
        assert np.all(vc[:, :, 4] == 1.0)                                  # the gait value of trot
        assert np.array_equal(vc[:, :, 1:3], np.broadcast_to(v_des[:, None, 0:2], (B, T, 2))) and np.array_equal(vc[:, :, 3], np.broadcast_to(w_des[:, None], (B, T)))


@pytest.mark.parametrize("goal_horizon", [1, 3])
def test_append_episodes_equals_the_host_database(goal_horizon):
    """a ring of 997 rows after two calls against dataset.Database fed the truncated episodes; episodes with a status bring no row"""
    import torch
    from bunmpc_amd import dataset
    from bunmpc_amd.dataset_device import DeviceDatabase
    rng = np.random.default_rng(5)
    db, host = DeviceDatabase(997, goal_horizon=goal_horizon, device=DEV, max_problems=64), dataset.Database(997, goal_horizon=goal_horizon)
    total = 0
    for call, T in enumerate((200, 130)):
        ee_pos, com = episodes(T)
        extra = cases.edges_log(T, [[], [17], [], []], 5)                  # one event in all: FEW_SWITCHES, no row
        ee_pos, com, start = np.concatenate([ee_pos, extra[0][None], ee_pos]), np.concatenate([com, extra[1][None], com]), STARTS + (5,) + STARTS
        B = len(start)
        g = dict(states=rng.normal(size=(B, T, 43)), actions=rng.normal(size=(B, T, 12)), vc_goals=rng.normal(size=(B, T, 5)))
        log = contact_log.DeviceContactLog(B, T, goal_horizon=goal_horizon, max_events=40, device=DEV)
        log.build(_dev(ee_pos), _dev(com), _dev(np.asarray(start), torch.int32), 400)
        db.append_episodes(_dev(g["states"]), _dev(g["actions"]), _dev(g["vc_goals"]), log)
        tw = contact_log.host_batch(ee_pos, com, start, 400, goal_horizon=goal_horizon, max_events=40)
        assert tw["status"][5] == contact_log.FEW_SWITCHES and np.all(np.delete(tw["status"], 5) == 0)
        for b in range(B):
            n = int(tw["rows"][b])
            if tw["status"][b] == 0 and n:
                host.append(g["states"][b, :n], g["actions"][b, :n], vc_goals=g["vc_goals"][b, :n], cc_goals=tw["goals"][b, :n])
                total += n
    assert total > 997                                                     # the ring has wrapped
    got = db.to_host()
    assert (got.start, got.length) == (host.start, host.length) == (total % 997, 997)
    for k in ("states", "vc_goals", "cc_goals", "actions"):
        assert np.array_equal(getattr(got, k), getattr(host, k)), k
