"""numpy twin of the contact-conditioned goal chain (include/bunmpc_goals.h, csrc/cc_goals.hip): plan, switches, schedule, estimated
CoM and goal rows as the reference computes them where a contact-conditioned policy is deployed (ISL/examples/iterative_algorithm/
simulation.py:999-1006 -> contact_planner.py:35-59, 61-256; utils.py:36-120, 187-219), written apart from bunmpc_amd/goals.py and
bunmpc_amd/contact_planner.py and without problems.contact_plan, so that the tests compare restatements that share no code.  The
plan is vectorised over the batch; switches and goal rows run problem by problem and row by row, literally: the scan over the
zero-padded schedule, the index past a foot's events that reads the padding, the index past N_total that ends the rows.

cc_goal_batch(...) returns what bmpc_cc_goal_batch_device leaves in its arrays, entry for entry."""
import numpy as np

FEW_SWITCHES, START_AFTER_END, PAST_SCHEDULE, EVENTS_OVERFLOW = 1, 2, 4, 8
WIDEN_Y = np.array([0.04, -0.04, 0.04, -0.04])


def plan_knots(gait, episode_length, sim_dt=0.001):
    return int(20.0 * episode_length * sim_dt * gait.gait_horizon * gait.gait_period / gait.gait_dt)      # contact_planner.py:130


def _phi(t, gait, j):
    return np.fmod(t + gait.phase_offset[j] * gait.gait_period, gait.gait_period)                          # gait_planner.cpp:41-44


def _in_stance(t, gait, j):
    st = gait.gait_period * gait.stance_percent[j]
    phi = _phi(t, gait, j)
    return (phi <= st) | (np.abs(phi - st) < 1e-4)                                                         # :46-58


def _percent(t, gait, j):
    st = gait.gait_period * gait.stance_percent[j]
    phi = _phi(t, gait, j)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(phi <= st, phi / st, (phi - st) / (gait.gait_period - st))                         # :112-128


def raibert_plan(gait, H, t0, com, feet0, hip_off, v_des, w_des):
    """contact_planner.py:61-234 for B problems: t0 (B,), com (B,3) and feet0 (B,4,3) unrounded, hip_off (B,4,2) yaw-rotated,
    v_des (B,3), w_des (B,) -> cnt_plan (B,H,4,4), swing_time (B,H,4)"""
    B = t0.shape[0]
    cnt, swing = np.zeros((B, H, 4, 4)), np.zeros((B, H, 4))
    c2, zh, v = np.round(com[:, 0:2], 3), com[:, 2], v_des[:, 0:2]
    a = 0.5 * np.sqrt(zh / 9.81)[:, None] * v
    ang = np.stack([a[:, 1] * w_des, -(a[:, 0] * w_des)], axis=1)
    for j in range(4):
        rb = 0.5 * v * gait.gait_period * gait.stance_percent[j] - 0.05 * (v - v)
        cnt[:, 0, j, 0] = _in_stance(t0, gait, j)
        cnt[:, 0, j, 1:4] = np.round(feet0[:, j], 3)
        for i in range(1, H):
            ft = np.round(t0 + i * gait.gait_dt, 3)
            on, was = _in_stance(ft, gait, j), cnt[:, i - 1, j, 0] == 1
            hip = c2 + hip_off[:, j] + i * gait.gait_dt * v
            per = np.round(_percent(ft, gait, j), 3)
            late = (per >= 0.5)[:, None]
            keep = (on & was)[:, None]
            xy = np.where(keep, cnt[:, i - 1, j, 1:3], np.where(on[:, None], rb + hip + ang, np.where(late, hip + ang + rb, hip + ang)))
            cnt[:, i, j, 0] = on
            cnt[:, i, j, 1:3] = xy
            cnt[:, i, j, 3] = np.where(keep[:, 0], cnt[:, i - 1, j, 3], 0.018)
            swing[:, i, j] = ~on & (per - 0.5 < 0.02)
    return cnt, swing


def switches(cnt_plan, start_step, gait_dt, sim_dt=0.001):
    """contact_planner.py:35-59 on one problem's plan (H,4,4): rows [ee, start_step + i gait_dt / sim_dt, x, y, 1e-3], (n, 5) -- always
    two-dimensional here (the reference returns [] or a 1-D row for n < 2, which its schedule code cannot take)"""
    rows = []
    for i in range(1, cnt_plan.shape[0]):
        for ee in range(cnt_plan.shape[1]):
            if cnt_plan[i, ee, 0] == 1 and cnt_plan[i - 1, ee, 0] != 1:
                rows.append([float(ee), start_step + i * gait_dt / sim_dt, cnt_plan[i, ee, 1], cnt_plan[i, ee, 2], 1e-3])
    return np.array(rows).reshape(-1, 5)


def schedule_of(sw, n_eff=4):
    """utils.py:104-120: (n_eff, N_total, 4) and the feet's counts"""
    out, count = np.zeros((n_eff, sw.shape[0], 4)), np.zeros(n_eff, dtype=int)
    for row in sw:
        ee = int(row[0])
        out[ee, count[ee]] = row[1:]
        count[ee] += 1
    return out, count


def contact_index(t, times):
    """utils.py:87-102 on a zero-padded row"""
    for sw in range(len(times) - 1):
        if t >= times[sw] and t < times[sw + 1]:
            return sw + 1
    return 0


def goal_rows(goal_length, sched, com_rows, goal_horizon, start_step):
    """utils.py:36-68 -> (rows written before the reference would raise (n, 12 goal_horizon), status).  Raises nothing: the status says
    what the reference does."""
    n_eff, N = sched.shape[0], sched.shape[1]
    end = goal_length
    for ee in range(n_eff):
        end = int(min(end, np.max(sched[ee, :, 0])))
    if start_step >= end:
        return np.zeros((0, 3 * n_eff * goal_horizon)), START_AFTER_END
    out = np.zeros((end - start_step, 3 * n_eff * goal_horizon))
    for t in range(start_step, end):
        r = t - start_step
        for gh in range(goal_horizon):
            for ee in range(n_eff):
                k = contact_index(t, sched[ee, :, 0]) + gh
                if k >= N:
                    return out[:r], PAST_SCHEDULE
                ev = sched[ee, k]
                s = 3 * n_eff * gh + 3 * ee
                out[r, s] = 1.0 * (ev[0] - t)
                out[r, s + 1:s + 3] = com_rows[r, 0:2] - ev[1:3]
    return out, 0


def estimated_com(com, v_des, n, sim_dt=0.001):
    """utils.py:187-219: (n, 3), z = 0"""
    out = np.zeros((n, 3))
    out[:, 0:2] = np.round(com, 3)[None, 0:2] + (np.arange(n) * sim_dt)[:, None] * v_des[None, 0:2]
    return out


def cc_goal_batch(gait, episode_length, goal_horizon, max_rows, max_events, t0, com, feet0, hip_off, v_des, w_des, com_rows=None, sim_dt=0.001):
    """the arrays of bmpc_cc_goal_batch_device: goals (B, max_rows, 12 goal_horizon), rows (B,), status (B,),
    schedule (B, 4, max_events, 4), counts (B, 4), cnt_plan, swing_time.  com_rows (B, max_rows, 3) or None: estimated."""
    B, H = t0.shape[0], plan_knots(gait, episode_length, sim_dt)
    cnt, swing = raibert_plan(gait, H, t0, com, feet0, hip_off, v_des, w_des)
    goals = np.zeros((B, max_rows, 12 * goal_horizon))
    rows, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    sched, counts = np.zeros((B, 4, max_events, 4)), np.zeros((B, 4), dtype=np.int32)
    for b in range(B):
        sw = switches(cnt[b], t0[b] / sim_dt, gait.gait_dt, sim_dt)
        s, c = schedule_of(sw)
        counts[b] = c
        for ee in range(4):
            m = min(c[ee], max_events)
            sched[b, ee, :m] = s[ee, :m]
        if sw.shape[0] > max_events:
            status[b] = EVENTS_OVERFLOW
        elif sw.shape[0] < 2:
            status[b] = FEW_SWITCHES
        else:
            start = int(t0[b] / sim_dt)                                                    # simulation.py:996
            cr = com_rows[b] if com_rows is not None else estimated_com(com[b], v_des[b], episode_length + 1, sim_dt)
            # rows the caller has no CoM for are never computed there: max_rows clips first
            out, status[b] = goal_rows_clipped(episode_length + 1, s, cr, goal_horizon, start, max_rows)
            rows[b] = out.shape[0]
            goals[b, :rows[b]] = out
    return dict(goals=goals, rows=rows, status=status, schedule=sched, counts=counts, cnt_plan=cnt, swing_time=swing)


def goal_rows_clipped(goal_length, sched, com_rows, goal_horizon, start_step, max_rows):
    """goal_rows with only max_rows CoM rows at hand: the status is that of the whole range [start_step, end_time), the rows are the
    leading ones (rows past max_rows are computed on zeros here and dropped)"""
    com = np.zeros((max(goal_length - start_step, com_rows.shape[0]), 3))
    com[:com_rows.shape[0]] = com_rows
    out, st = goal_rows(goal_length, sched, com, goal_horizon, start_step)
    return out[:max_rows], st


def front_end(model, x, feet, hips):
    """contact_planner.py:80-124 for B states x (B,37): com (B,3), feet0 (B,4,3), hips (B,4,3) unrounded, hip_off (B,4,2), and
    `pre`: every value that is rounded to 3 decimals on the way (for the tie check of the end-to-end test)"""
    from bunmpc_amd import fk_np
    kin = fk_np.kinematics(model, x[:, :19])
    com = kin["com"]
    f, h = fk_np.frame_positions(model, kin, feet), fk_np.frame_positions(model, kin, hips)
    R = kin["oR"][0]
    rel = h - com[:, None, :]
    o = np.round(rel, 3)
    o[:, :, 1] += WIDEN_Y[None]
    ob = np.einsum("bki,bjk->bji", R, o)                   # R^T o
    yaw = np.arctan2(R[:, 1, 0], R[:, 0, 0])
    c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    hip_off = np.stack([c * ob[:, :, 0] - s * ob[:, :, 1], s * ob[:, :, 0] + c * ob[:, :, 1]], axis=2)
    pre = np.concatenate([com[:, 0:2].reshape(-1), f.reshape(-1), rel.reshape(-1)])
    return dict(com=com, feet0=f, hips=h, hip_off=hip_off, pre=pre)


def distance_to_rounding_tie(v):
    """how far each value is from the nearest k + 0.5 thousandths, in its own units"""
    m = np.asarray(v) * 1000.0
    return np.abs(m - np.floor(m) - 0.5) / 1000.0


def reference_goal(goal_length, sw, com_rows, goal_horizon, start_step, n_eff=4):
    """the goal array as the reference returns it, raising where the reference raises: fewer than two switches (no schedule),
    start_step > end_time (an array of negative length), an index past N_total"""
    if np.ndim(sw) < 2 or np.shape(sw)[0] < 2:
        raise IndexError("fewer than two switches: no contact schedule")
    sched, _ = schedule_of(np.asarray(sw), n_eff)
    end = goal_length
    for ee in range(n_eff):
        end = int(min(end, np.max(sched[ee, :, 0])))
    if start_step > end:
        raise ValueError("start_step %d after end_time %d" % (start_step, end))
    out, status = goal_rows(goal_length, sched, com_rows, goal_horizon, start_step)
    if status == PAST_SCHEDULE:
        raise IndexError("goal index past the %d switches of the schedule" % sched.shape[1])
    return out


SOLO12_Q0 = np.array([0, 0, 0.2409, 0, 0, 0, 1] + [0, 0.8, -1.6] * 2 + [0, -0.8, 1.6] * 2, float)      # problems.SOLO12_Q0


def wb_states(B, seed=19):
    """Solo12 states x (B,37) with yawed (up to +-1.5 rad), pitched and rolled bases, unit quaternions.  The default seed is one whose
    five states keep every rounded value 8e-6 away from a rounding tie (tests/test_cc_goals_cpu.py asserts > 1e-6)"""
    rng = np.random.default_rng(seed)
    q = np.tile(SOLO12_Q0, (B, 1))
    q[:, 0:2] = rng.normal(0, 0.3, (B, 2))
    q[:, 2] += rng.normal(0, 0.01, B)
    yaw, pitch, roll = rng.uniform(-1.5, 1.5, B), rng.normal(0, 0.15, B), rng.normal(0, 0.1, B)
    for b in range(B):
        qz = np.array([0, 0, np.sin(yaw[b] / 2), np.cos(yaw[b] / 2)])
        qy = np.array([0, np.sin(pitch[b] / 2), 0, np.cos(pitch[b] / 2)])
        qx = np.array([np.sin(roll[b] / 2), 0, 0, np.cos(roll[b] / 2)])
        qq = quat_mul(quat_mul(qz, qy), qx)
        q[b, 3:7] = qq / np.linalg.norm(qq)
    q[:, 7:] += rng.normal(0, 0.05, (B, 12))
    return np.concatenate([q, rng.normal(0, 0.1, (B, 18))], axis=1)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])
