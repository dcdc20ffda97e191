"""Measured contact goals without a GPU: the host functions of bunmpc_amd/contact_log.py against recorded outputs of the reference's own
functions (tests/golden/contact_log/contact_log_ref.npz, made by tests/golden/make_golden_contact_log.py), the quirks of the reference's
loop against a second statement of its semantics on whole arrays, the batch twin (host_batch) against the per-episode functions, include/ext/bunmpc_contact_log.h
against its recorded table and a C compiler, and every refusal of bmpc_contact_log_goals_device (they return before any launch)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from bunmpc_amd import _lib, _lib_contact_log, contact_log, goals
from bunmpc_amd import build as hip_build
from tests import contact_log_cases as cases
from tests.test_abi_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_abi  # noqa: E402

EXT = os.path.dirname(_lib_contact_log.HEADER)
REF = np.load(os.path.join(ROOT, "tests", "golden", "contact_log", "contact_log_ref.npz"))
NAMES = [str(n) for n in REF["names"]]
HORIZONS = cases.FIXTURE_HORIZONS
LOGS = cases.fixture_logs()      # the inputs of the recording, made again: the recorded switches and goals pin them


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def log(i):
    name, ee_pos, com, start, length = LOGS[i]
    assert (name, start, length) == (NAMES[i], int(REF["l%d_start_step" % i]), int(REF["l%d_episode_length" % i]))
    return ee_pos, com, start, length


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------

def test_fixture_holds_the_cases_the_recipe_names():
    assert NAMES == ["trot0", "trot7", "bound0", "bound130", "jump0", "jump370", "two_events", "one_event", "start_after_end", "past_schedule"]
    raised = {(n, gh): int(REF["l%d_h%d_raised" % (i, gh)]) for i, n in enumerate(NAMES) for gh in HORIZONS.get(n, (1, 3))}
    assert raised[("past_schedule", 5)] == 2 and raised[("start_after_end", 1)] == 1 and raised[("two_events", 3)] == 0
    assert sum(v == 0 for v in raised.values()) == 18 and int(REF["l7_sched_raised"]) == 1
    assert len(REF["l6_switches"]) == 2 and len(REF["l7_switches"]) == 1 and REF["quat"].shape == (50, 4)
    assert any(length < start + len(ee_pos) for _, ee_pos, _, start, length in LOGS)


@pytest.mark.parametrize("i", range(len(NAMES)))
def test_switches_edges_and_schedule_equal_the_recorded_ones(i):
    ee_pos, com, start, length = log(i)
    used = max(0, min(len(ee_pos), length - start))
    sw = contact_log.measured_switches(ee_pos[:used], start)
    assert same(np.asarray(sw, float).reshape(-1, 5), REF["l%d_switches" % i])
    assert (np.ndim(sw), len(sw)) == ((2, len(sw)) if len(REF["l%d_switches" % i]) > 1 else (1, 5) if len(REF["l%d_switches" % i]) else (1, 0))
    got, pre = np.zeros((used, 4), np.int8), np.zeros((4, 3))
    for r in range(used):      # the answers of the reference's Simulation.new_ee_contact, recorded row by row
        got[r, contact_log.rising_feet(ee_pos[r], pre)] = 1
        pre = ee_pos[r]
    assert same(np.packbits(got, axis=None), REF["l%d_new_ee" % i])
    if int(REF["l%d_sched_raised" % i]):
        with pytest.raises((TypeError, IndexError)):
            goals.construct_contact_schedule(sw, 4)
    else:
        assert same(goals.construct_contact_schedule(sw, 4), REF["l%d_schedule" % i])


@pytest.mark.parametrize("i,gh", [(i, gh) for i, n in enumerate(NAMES) for gh in HORIZONS.get(n, (1, 3))])
def test_measured_cc_goals_equal_the_recorded_ones_and_raise_what_was_recorded(i, gh):
    ee_pos, com, start, length = log(i)
    raised = int(REF["l%d_h%d_raised" % (i, gh)])
    if int(REF["l%d_sched_raised" % i]):
        with pytest.raises((TypeError, IndexError)):
            contact_log.measured_cc_goals(ee_pos, com, length, start, gh)
    elif raised:
        with pytest.raises({1: ValueError, 2: IndexError}[raised]):
            contact_log.measured_cc_goals(ee_pos, com, length, start, gh)
    else:
        schedule, goal = contact_log.measured_cc_goals(ee_pos, com, length, start, gh)
        assert same(schedule, REF["l%d_schedule" % i]) and same(goal, REF["l%d_h%d_goal" % (i, gh)])


def test_euler_angles_equal_the_recorded_ones():
    got = np.array([contact_log.quaternion_to_euler_angle(*(float(a) for a in q)) for q in REF["quat"]])
    assert same(got, REF["euler"])
    assert got[1, 1] == 90.0 and got[2, 1] == -90.0      # asin at 1, and the clamp


# ---- the loop's quirks, against a second statement of the loop's semantics (simulation.py:437-550), on whole arrays -------------------------

def loop(ee_pos_log, start_step, episode_length):
    """What the rollout loop leaves in its list of new contacts, said with array operations and not row by row: a foot is in contact
    where |x| > 1e-12 and cleared where |x| <= 1e-12 (two masks, not complements: a NaN is in neither); it rises at a row that is in
    contact after a cleared row, "cleared" standing before row 0; the rise at absolute step 0 is dropped; events are ordered by row,
    then by foot, as [foot, step, x, y, z]; none gives [], one a 1-D array, more an (n, 5) array."""
    log = np.asarray(ee_pos_log, float)[:max(0, episode_length - start_step)]
    with np.errstate(invalid="ignore"):
        contact, cleared = np.abs(log[:, :, 0]) > 1e-12, np.abs(log[:, :, 0]) <= 1e-12
    rises = contact & np.vstack([np.ones((1, log.shape[1]), bool), cleared[:-1]])
    steps = start_step + np.arange(len(log))
    rises[steps == 0] = False
    at = np.argwhere(rises)      # row-major: rows ascending, feet ascending within a row
    events = np.column_stack([at[:, 1], steps[at[:, 0]], log[at[:, 0], at[:, 1]]]).astype(float) if len(at) else np.zeros((0, 5))
    return [] if len(events) == 0 else events[0] if len(events) == 1 else events


def quirk_logs():
    """{name: (ee_pos (T, 4, 3), start_step, the steps of foot 0's events)}"""
    above = np.nextafter(1e-12, 1.0)
    out = {}
    ee = np.zeros((12, 4, 3))
    ee[0:3, 0] = ee[6:9, 0] = [0.2, 0.1, 0.0]
    ee[:, 1] = [0.3, 0.0, 0.0]
    out["o == 0 is skipped"] = (ee.copy(), 0, [6])                        # feet 0 and 1 stand at row 0 = step 0: not recorded
    out["start_step 7 records the feet standing at row 0"] = (ee.copy(), 7, [7, 13])
    ee = np.zeros((10, 4, 3))
    ee[2:5, 0] = [0.0, 0.4, 0.01]                                         # in contact at x == 0.0: no contact
    ee[7, 0] = [0.1, 0.4, 0.01]
    out["x == 0.0 in contact"] = (ee, 0, [7])
    ee = np.zeros((10, 4, 3))
    ee[2, 0, 0], ee[4, 0, 0], ee[6, 0, 0], ee[8, 0, 0] = 1e-12, above, -1e-12, -above
    out["|x| of 1e-12 is no contact, the next double is"] = (ee, 0, [4, 8])
    ee = np.zeros((10, 4, 3))
    ee[3, 0] = [np.nan, 0.1, 0.1]                                         # neither a contact at row 3 nor a cleared predecessor for row 4
    ee[4:6, 0] = [0.2, 0.1, 0.0]
    ee[8, 0] = [0.2, np.nan, 0.0]                                         # a NaN beside x goes into the event
    out["a NaN x"] = (ee, 0, [8])
    return out


@pytest.mark.parametrize("name", list(quirk_logs()))
def test_quirks_of_the_loop(name):
    ee, start, steps = quirk_logs()[name]
    ref = loop(ee, start, start + len(ee))
    got = contact_log.measured_switches(ee, start)
    assert same(got, ref) and np.ndim(got) == np.ndim(ref)
    rows = np.asarray(ref, float).reshape(-1, 5)
    assert [int(o) for o in rows[rows[:, 0] == 0][:, 1]] == steps
    tw = contact_log.host_batch(ee[None], np.zeros((1, len(ee), 3)), [start], start + len(ee), max_events=8)
    for j in range(4):
        mine = rows[rows[:, 0] == j][:, 1:]
        assert tw["counts"][0, j] == len(mine) and same(tw["schedule"][0, j, :len(mine)], mine) and not tw["schedule"][0, j, len(mine):].any()


@pytest.mark.parametrize("i", range(len(NAMES)))
def test_loop_restatement_equals_the_recorded_switches(i):
    ee_pos, com, start, length = log(i)
    assert same(np.asarray(loop(ee_pos, start, min(length, start + len(ee_pos))), float).reshape(-1, 5), REF["l%d_switches" % i])


# ---- the batch twin against the per-episode functions -----------------------------------------------------------------------------------

@pytest.mark.parametrize("i,gh", [(i, gh) for i, n in enumerate(NAMES) for gh in HORIZONS.get(n, (1, 3))])
def test_host_batch_equals_the_per_episode_functions(i, gh):
    ee_pos, com, start, length = log(i)
    T = len(ee_pos)
    tw = contact_log.host_batch(ee_pos[None], com[None], [start], length, goal_horizon=gh, max_events=32)
    raised = int(REF["l%d_h%d_raised" % (i, gh)])
    status, rows = int(tw["status"][0]), int(tw["rows"][0])
    assert tw["goals"].shape == (1, T, 12 * gh) and not tw["goals"][0, rows:].any() and tw["failed_step"][0] == -1
    if int(REF["l%d_sched_raised" % i]):
        assert (status, rows) == (contact_log.FEW_SWITCHES, 0)
    elif raised == 1:
        assert (status, rows) == (contact_log.START_AFTER_END, 0)
    elif raised == 2:
        assert status == contact_log.PAST_SCHEDULE and rows == 60      # foot 0's sixth event: index 6 + 4 reaches N_total = 10
        assert same(tw["goals"][0, :rows, :36], REF["l%d_h3_goal" % i][:rows])      # the rows before it, as the lower horizon has them
    else:
        goal = REF["l%d_h%d_goal" % (i, gh)]
        assert status == 0 and rows == len(goal) and same(tw["goals"][0, :rows], goal)
    if not int(REF["l%d_sched_raised" % i]):
        n = len(REF["l%d_switches" % i])
        assert same(tw["schedule"][0, :, :n], REF["l%d_schedule" % i]) and not tw["schedule"][0, :, n:].any() and tw["counts"][0].sum() == n


def test_host_batch_clips_rows_and_flags_an_overflow():
    ee_pos, com, start, length = log(0)
    tw = contact_log.host_batch(ee_pos[None], com[None], [start], length, max_events=32, max_rows=40)
    assert tw["rows"][0] == 40 and same(tw["goals"][0], REF["l0_h1_goal"][:40])
    tw = contact_log.host_batch(ee_pos[None], com[None], [start], length, max_events=13)      # 14 switches
    assert (tw["status"][0], tw["rows"][0]) == (contact_log.EVENTS_OVERFLOW, 0) and tw["counts"][0].sum() == 14 and not tw["goals"].any()


def test_failed_states_and_the_twin_agree():
    q = np.zeros((1, 30, 19))
    q[:, :, 2], q[:, :, 6] = 0.23, 1.0
    q[0, 5, 2] = 0.01                                   # within the grace rows: not a failure
    q[0, 20, 3:7] = cases.quaternion_xyzw(31.0, 0.0)
    q[0, 25, 2] = 0.01
    ee_pos, com, start, length = log(0)
    tw = contact_log.host_batch(ee_pos[None, :30], com[None, :30], [0], 30, q=q, grace=10.0)
    assert tw["failed_step"][0] == 20 and tw["status"][0] & contact_log.FAILED_STATE and tw["rows"][0] == 0 and not tw["goals"].any()
    flags = [contact_log.failed_states(q[0, r], r, 0.01, 0.001, lax=False) for r in range(30)]
    assert [r for r in range(30) if flags[r]] == [20, 25]
    assert abs(tw["angles"][0, 20, 0] - 31.0) < 1e-12 and tw["angles"][0, 0, 0] == 0.0
    # the height thresholds are strict, and lax moves the lower one
    low = np.array([0, 0, 0.1, 0, 0, 0, 1.0])
    assert not contact_log.failed_states(low, 11, 0.01, 0.001, lax=False) and contact_log.failed_states(low - [0, 0, 0.01, 0, 0, 0, 0], 11, 0.01, 0.001, lax=False)
    assert not contact_log.failed_states(low - [0, 0, 0.05, 0, 0, 0, 0], 11, 0.01, 0.001, lax=True)
    assert not contact_log.failed_states(low - [0, 0, 0.09, 0, 0, 0, 0], 10, 0.01, 0.001, lax=False)      # time_elapsed == grace


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def test_header_equals_its_recorded_table():
    with open(os.path.join(ROOT, "tests", "golden", "abi_contact_log.json")) as f:
        assert record_abi.dump(_lib_contact_log.ABI) == f.read()
    assert sorted(_lib_contact_log.ABI.functions) == ["bmpc_contact_log_goals_device", "bmpc_contact_log_struct_size"]
    d = _lib_contact_log.ABI.defines
    assert [d["BMPC_CL_" + n] for n in ("FEW_SWITCHES", "START_AFTER_END", "PAST_SCHEDULE", "EVENTS_OVERFLOW", "FAILED_STATE")] == [1, 2, 4, 8, 16]
    assert (contact_log.FEW_SWITCHES, contact_log.START_AFTER_END, contact_log.PAST_SCHEDULE, contact_log.EVENTS_OVERFLOW, contact_log.FAILED_STATE) == (1, 2, 4, 8, 16)


def test_header_lives_under_ext_and_its_unit_is_a_row_of_the_job_table():
    assert _lib_contact_log.HEADER in hip_build.dependencies() and "bunmpc_contact_log.h" not in _lib.HEADER_NAMES
    assert not set(_lib_contact_log.ABI.functions) & set(_lib._SIGS) and not set(_lib_contact_log.ABI.structs) & set(_lib._ABI.structs)
    assert ("contact_log", "contact_log.hip", []) in hip_build.compile_jobs()[12:]
    assert _lib_contact_log.lib().bmpc_contact_log_struct_size() == C.sizeof(_lib_contact_log.ContactLog)


def test_a_c_compiler_lays_the_struct_out_as_ctypes_does(tmp_path):
    cc = _compiler()
    if cc is None:
        pytest.skip("no C compiler on this machine")
    want, lines = [], []
    for cname, cls in _lib_contact_log.ABI.structs.items():
        want.append("%s %d" % (cname, C.sizeof(cls)))
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            want.append("%s.%s %d %d" % (cname, field, getattr(cls, field).offset, getattr(cls, field).size))
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, field, cname, field, cname, field))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bunmpc_contact_log.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", EXT, "-o", str(tmp_path / "layout"), str(src)])
    assert subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")[:-1] == want
    for lang in ("c", "c++"):      # alone, as C and as C++; and it includes nothing
        subprocess.check_call([cc, "-x", lang, "-fsyntax-only", "-Wall", "-Werror", _lib_contact_log.HEADER])
    assert "#include" not in open(_lib_contact_log.HEADER).read()
    both = tmp_path / "both.c"      # and beside the first header and the others under ext/
    both.write_text('#include "bunmpc.h"\n#include "ext/bunmpc_dataset.h"\n#include "ext/bunmpc_contact_log.h"\nint main(void) { return 0; }\n')
    subprocess.check_call([cc, "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.dirname(hip_build.INCLUDE), str(both)])


# ---- refusals: before anything is written or launched, so they need no GPU ----------------------------------------------------------------

def _desc(**kw):
    """a descriptor that passes every check (its arrays are never touched: every call below is refused), with fields replaced"""
    d = _lib_contact_log.ContactLog()
    d.B, d.T, d.n_eff, d.goal_horizon, d.max_events, d.max_rows, d.episode_length, d.check_failed = 8, 200, 4, 3, 32, 150, 3000, 1
    d.z_min, d.fail_angle, d.grace, d.s_q = 0.1, 30.0, 500.0, 37
    for k in ("start_step", "ee_pos", "com", "q", "schedule", "counts", "goals", "rows", "status", "failed_step", "angles"):
        setattr(d, k, 4096)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


_REFUSALS = [(dict(B=-1), "B must be"), (dict(B=(1 << 20) + 1), "B must be"), (dict(T=0), "T must be"), (dict(T=(1 << 20) + 1), "T must be"),
             (dict(episode_length=0), "episode_length"), (dict(episode_length=(1 << 20) + 1), "episode_length"), (dict(max_rows=0), "max_rows"),
             (dict(max_rows=201), "max_rows"), (dict(goal_horizon=0), "goal_horizon"), (dict(goal_horizon=65), "goal_horizon"), (dict(n_eff=2), "n_eff"),
             (dict(max_events=1), "max_events"), (dict(max_events=(1 << 16) + 1), "max_events"),
             (dict(B=1 << 20, T=1 << 20, max_rows=1), "ee_pos of more than 2^40"), (dict(B=1 << 20, T=1 << 10, max_rows=1, s_q=1 << 10), "q of more than 2^40"),
             (dict(B=1 << 20, T=1 << 12, max_rows=1 << 12, goal_horizon=64, s_q=19), "goals of more than 2^40"),
             (dict(B=1 << 20, max_events=1 << 16), "schedule of more than 2^40"),
             (dict(B=1 << 20, T=1 << 12, max_rows=1 << 12, goal_horizon=1, s_q=19), "one thread per goal slot"),
             (dict(B=1 << 20, T=1 << 12, max_rows=1, s_q=19), "one thread per row"),
             (dict(start_step=None), "start_step"), (dict(ee_pos=None), "ee_pos"), (dict(com=None), "com"), (dict(schedule=None), "schedule"),
             (dict(counts=None), "counts"), (dict(goals=None), "goals"), (dict(rows=None), "rows"), (dict(status=None), "status"),
             (dict(q=None), "q (check_failed"), (dict(s_q=18), "s_q"), (dict(fail_angle=float("nan")), "fail_angle"), (dict(fail_angle=float("inf")), "fail_angle"),
             (dict(z_min=float("-inf")), "z_min"), (dict(grace=float("nan")), "grace")]


@pytest.mark.parametrize("kw,word", _REFUSALS)
def test_every_refusal_names_its_field(kw, word):
    rc = _lib_contact_log.lib().bmpc_contact_log_goals_device(C.byref(_desc(**kw)), None)
    assert rc == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()


def test_null_descriptor_is_refused_and_optional_arrays_are_optional():
    lib = _lib_contact_log.lib()
    assert lib.bmpc_contact_log_goals_device(None, None) == _lib.BAD_ARG and "null contact log descriptor" in _lib.last_error()
    # B == 0 passes the checks and launches nothing: failed_step, angles and (without check_failed) q may be NULL
    assert lib.bmpc_contact_log_goals_device(C.byref(_desc(B=0, failed_step=None, angles=None, q=None, check_failed=0, s_q=0)), None) == _lib.OK
