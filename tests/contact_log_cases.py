"""Synthetic contact logs for the measured-goal tests (not a test module): what a rollout would have logged -- contact positions per
step (zeros for a foot in the air) and the CoM -- for the trot, bound and jump contact patterns, with short gait periods so that a log of
200 rows holds many touchdowns.  Deterministic on any machine: integer arithmetic and divisions by powers of two, no random state and no
library function, so the logs behind the recorded fixture can be made again bit for bit."""
import numpy as np

PATTERNS = {"trot": (0, 2, 2, 0), "bound": (0, 0, 2, 2), "jump": (0, 0, 0, 0)}      # phase offsets of FL, FR, HL, HR in quarter periods
HIPS = np.array([[25, 19], [25, -19], [-25, 19], [-25, -19]]) / 128.0


def synthetic_log(pattern, T, start_step, period=50, stance=0.6):
    """(ee_pos (T, 4, 3), com (T, 3)) of steps start_step .. start_step + T - 1: foot j stands while its phase is below `stance`"""
    ee, com = np.zeros((T, 4, 3)), np.zeros((T, 3))
    off = PATTERNS[pattern]
    for r in range(T):
        o = start_step + r
        com[r] = [3 * o / 8192.0 + (o * 37 % 101) / 65536.0, (o * 53 % 89) / 65536.0 - 1 / 128.0, 0.23 + (o * 11 % 13) / 8192.0]
        for j in range(4):
            ticks = 4 * o + off[j] * period          # the phase in units of a quarter step
            cycle, phase = divmod(ticks, 4 * period)
            if phase < stance * 4 * period:
                wobble = ((13 * j + 29 * cycle) % 17) / 2048.0
                ee[r, j] = [HIPS[j, 0] + 3 * period * cycle / 8192.0 + wobble, HIPS[j, 1] - wobble / 2, (1 + j) / 1024.0]
    return ee, com


def edges_log(T, rows_by_foot, start_step=0):
    """a log whose foot j touches down exactly at the rows rows_by_foot[j] (one row of contact each, unless the next row is a touchdown
    row too, which would not be an edge: such rows are asserted against)"""
    ee, com = np.zeros((T, 4, 3)), np.zeros((T, 3))
    for j, rows in enumerate(rows_by_foot):
        for r in rows:
            assert r - 1 not in rows
            ee[r, j] = [(100 + r) / 1024.0 + j / 128.0, j / 1024.0 - 25 / 128.0, 1 / 1024.0]
    for r in range(T):
        com[r] = [(start_step + r) / 1024.0, -r / 8192.0, 0.23]
    return ee, com


def quaternion_xyzw(roll_deg, pitch_deg, yaw_deg=0.0):
    """(x, y, z, w) of the ZYX Euler angles, in degrees"""
    r, p, y = np.radians(roll_deg) / 2, np.radians(pitch_deg) / 2, np.radians(yaw_deg) / 2
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


FIXTURE_HORIZONS = {"past_schedule": (1, 3, 5)}      # goal horizons recorded per fixture log, (1, 3) where not named


def fixture_logs():
    """[(name, ee_pos, com, start_step, episode_length)]: the logs whose outputs tests/golden/contact_log/contact_log_ref.npz records.
    The file holds the outputs alone; a change here shows as a mismatch of the recorded switches and goals."""
    out = []
    for name, pattern, T, start, length in (("trot0", "trot", 96, 0, 96), ("trot7", "trot", 96, 7, 90), ("bound0", "bound", 80, 0, 3000),
                                            ("bound130", "bound", 72, 130, 202), ("jump0", "jump", 96, 0, 80), ("jump370", "jump", 64, 370, 434)):
        out.append((name,) + synthetic_log(pattern, T, start, period=24) + (start, length))
    out.append(("two_events",) + edges_log(60, [[20], [], [31], []]) + (0, 60))
    out.append(("one_event",) + edges_log(40, [[], [17], [], []], 5) + (5, 45))
    out.append(("start_after_end",) + edges_log(30, [[3, 9], [], [5], [12]], 7) + (7, 37))
    out.append(("past_schedule",) + edges_log(100, [[10, 20, 30, 40, 50, 60, 95], [90], [91], [92]]) + (0, 100))
    return out
