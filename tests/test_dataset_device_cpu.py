"""include/ext/bunmpc_dataset.h without a GPU: the header against its recorded table and a C compiler, the refusals of its three calls
(they return before any launch), and the twin (tests/dataset_np.py) held to the reference's row-by-row loop, to
bunmpc_amd/dataset.py::Database and to exact rational arithmetic -- and shown to fail, with one fault planted, the comparisons the GPU
tests apply."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from bunmpc_amd import _lib, _lib_dataset, dataset
from bunmpc_amd import build as hip_build
from tests import dataset_np as twin
from tests.test_abi_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_abi  # noqa: E402

EXT = os.path.dirname(_lib_dataset.HEADER)


# ---- the header -----------------------------------------------------------------------------------------------------------------------

def test_header_equals_its_recorded_table():
    with open(os.path.join(ROOT, "tests", "golden", "abi_dataset.json")) as f:
        assert record_abi.dump(_lib_dataset.ABI) == f.read()
    assert sorted(_lib_dataset.ABI.functions) == ["bmpc_dataset_append_device", "bmpc_dataset_batch_device", "bmpc_dataset_batch_struct_size",
                                                  "bmpc_dataset_moments_device", "bmpc_dataset_rows_struct_size", "bmpc_dataset_scratch_bytes",
                                                  "bmpc_dataset_struct_size"]
    assert (_lib_dataset.STATE_WIDTH, _lib_dataset.VC_WIDTH, _lib_dataset.ACTION_WIDTH) == (dataset.STATE_WIDTH, dataset.VC_GOAL_WIDTH, dataset.ACTION_WIDTH)


def test_header_lives_under_ext_and_makes_the_library_stale():
    assert _lib_dataset.HEADER in hip_build.dependencies() and "bunmpc_dataset.h" not in _lib.HEADER_NAMES
    assert not set(_lib_dataset.ABI.functions) & set(_lib._SIGS) and not set(_lib_dataset.ABI.structs) & set(_lib._ABI.structs)
    jobs = hip_build.compile_jobs()
    assert ("dataset", "dataset.hip", []) in jobs[12:] and all(j[1] == "biconvex_admm.hip" for j in jobs[:12])
    lib = _lib_dataset.lib()      # the symbols are in the library, with the header's struct sizes
    assert lib.bmpc_dataset_struct_size() == C.sizeof(_lib_dataset.Dataset) and lib.bmpc_dataset_rows_struct_size() == C.sizeof(_lib_dataset.DatasetRows)
    assert lib.bmpc_dataset_batch_struct_size() == C.sizeof(_lib_dataset.DatasetBatch)


def test_a_c_compiler_lays_the_structs_out_as_ctypes_does(tmp_path):
    cc = _compiler()
    if cc is None:
        pytest.skip("no C compiler on this machine")
    want, lines = [], []
    for cname, cls in _lib_dataset.ABI.structs.items():
        want.append("%s %d" % (cname, C.sizeof(cls)))
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            want.append("%s.%s %d %d" % (cname, field, getattr(cls, field).offset, getattr(cls, field).size))
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, field, cname, field, cname, field))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bunmpc_dataset.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", EXT, "-o", str(tmp_path / "layout"), str(src)])
    assert subprocess.check_output([str(tmp_path / "layout")], text=True).split("\n")[:-1] == want
    for lang in ("c", "c++"):      # alone, as C and as C++; and it includes nothing
        subprocess.check_call([cc, "-x", lang, "-fsyntax-only", "-Wall", "-Werror", _lib_dataset.HEADER])
    assert "#include" not in open(_lib_dataset.HEADER).read()
    both = tmp_path / "both.c"      # and beside the first header and the other one under ext/
    both.write_text('#include "bunmpc.h"\n#include "ext/bunmpc_acyclic.h"\n#include "ext/bunmpc_dataset.h"\nint main(void) { return 0; }\n')
    subprocess.check_call([cc, "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.dirname(hip_build.INCLUDE), str(both)])


# ---- refusals: before anything is written or launched, so they need no GPU --------------------------------------------------------------

def _set(d, kw):
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _ds(**kw):
    """a descriptor that passes every check (its arrays are never touched: every call below is refused), with fields replaced"""
    d = _lib_dataset.Dataset()
    d.limit, d.max_problems = 1000, 64
    d.w_states, d.w_vc, d.w_cc, d.w_actions = 43, 5, 12, 12
    d.states = d.vc_goals = d.cc_goals = d.actions = d.header = d.scratch = 4096
    w_cc = kw.get("w_cc", 12)
    d.scratch_bytes = max(_lib_dataset.lib().bmpc_dataset_scratch_bytes(1000, w_cc if 0 <= w_cc <= 768 and w_cc % 3 == 0 else 12, 64), 0)
    return _set(d, kw)


def _rows(**kw):
    r = _lib_dataset.DatasetRows()
    r.B, r.R = 8, 50
    r.w_states, r.w_vc, r.w_cc, r.w_actions = 43, 5, 12, 12
    r.states = r.actions = r.vc_goals = r.cc_goals = r.rows = r.keep = 4096
    return _set(r, kw)


def _batch(**kw):
    q = _lib_dataset.DatasetBatch()
    q.n, q.goal_type, q.normalise = 16, _lib_dataset.GOAL["cc"], 1
    q.index = q.states_mean = q.states_std = q.goal_mean = q.goal_std = q.x = q.y = 4096
    return _set(q, kw)


_DS_REFUSALS = [(dict(limit=0), "limit"), (dict(limit=1 << 31), "limit"), (dict(w_states=42), "w_states"), (dict(w_vc=4), "w_vc"),
                (dict(w_actions=13), "w_actions"), (dict(w_cc=13), "w_cc"), (dict(w_cc=-3), "w_cc"), (dict(w_cc=771), "w_cc"),
                (dict(max_problems=0), "max_problems"), (dict(max_problems=(1 << 24) + 1), "max_problems"), (dict(states=None), "states"),
                (dict(vc_goals=None), "vc_goals"), (dict(cc_goals=None), "cc_goals"), (dict(actions=None), "actions"), (dict(header=None), "header"),
                (dict(scratch=None), "scratch"), (dict(scratch=4104), "scratch"), (dict(scratch_bytes=16), "scratch_bytes")]


def _calls(ds):
    lib, f = _lib_dataset.lib(), 4096
    return [lambda: lib.bmpc_dataset_append_device(ds, C.byref(_rows()), None),
            lambda: lib.bmpc_dataset_moments_device(ds, f, f, f, f, None),
            lambda: lib.bmpc_dataset_batch_device(ds, C.byref(_batch()), None)]


@pytest.mark.parametrize("kw,word", _DS_REFUSALS)
def test_every_call_refuses_a_bad_data_set_and_names_the_field(kw, word):
    for call in _calls(C.byref(_ds(**kw))):
        assert call() == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()


def test_null_descriptors_are_refused():
    lib = _lib_dataset.lib()
    for call in _calls(None):
        assert call() == _lib.BAD_ARG and "null data set descriptor" in _lib.last_error()
    assert lib.bmpc_dataset_append_device(C.byref(_ds()), None, None) == _lib.BAD_ARG and "rows descriptor" in _lib.last_error()
    assert lib.bmpc_dataset_batch_device(C.byref(_ds()), None, None) == _lib.BAD_ARG and "batch descriptor" in _lib.last_error()
    assert lib.bmpc_dataset_scratch_bytes(0, 12, 64) == -1 and lib.bmpc_dataset_scratch_bytes(1000, 13, 64) == -1
    assert lib.bmpc_dataset_scratch_bytes(1000, 12, 0) == -1 and lib.bmpc_dataset_scratch_bytes(1 << 31, 12, 64) == -1
    # counts (int) and offsets (long) per problem, two longs per chunk of the prefix, the total, and one partial per 1024 rows and column
    assert lib.bmpc_dataset_scratch_bytes(1000, 12, 64) == 64 * 4 + 64 * 8 + 16 + 16 + 16 + 43 * 8 + 8 + 12 * 8
    assert lib.bmpc_dataset_scratch_bytes((1 << 31) - 1, 768, 1 << 24) > 0


@pytest.mark.parametrize("kw,word", [(dict(B=-1), "B must be"), (dict(B=65), "B must be"), (dict(R=0), "R must be"), (dict(R=1 << 22), "R must be"), (dict(w_states=44), "w_states"),
                                     (dict(w_vc=6), "w_vc"), (dict(w_cc=36), "w_cc"), (dict(w_actions=11), "w_actions"), (dict(states=None), "states"),
                                     (dict(actions=None), "actions"), (dict(vc_goals=None, cc_goals=None), "both vc_goals and cc_goals")])
def test_append_refusals_name_the_field(kw, word):
    rc = _lib_dataset.lib().bmpc_dataset_append_device(C.byref(_ds()), C.byref(_rows(**kw)), None)
    assert rc == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()


def test_append_refuses_too_many_rows_and_cc_goals_without_the_group():
    lib = _lib_dataset.lib()
    big = _ds(max_problems=1 << 24)
    big.scratch_bytes = lib.bmpc_dataset_scratch_bytes(1000, 12, 1 << 24)
    assert lib.bmpc_dataset_append_device(C.byref(big), C.byref(_rows(B=1 << 24, R=128)), None) == _lib.BAD_ARG and "B R" in _lib.last_error()
    assert lib.bmpc_dataset_append_device(C.byref(_ds(w_cc=0, cc_goals=None)), C.byref(_rows(w_cc=0)), None) == _lib.BAD_ARG
    assert "cc_goals" in _lib.last_error() and "without that group" in _lib.last_error()


def test_moments_refusals_name_the_field():
    lib, f = _lib_dataset.lib(), 4096
    for args, word in (((None, f, f, f), "states_mean"), ((f, None, f, f), "states_std"), ((f, f, None, f), "cc_mean"), ((f, f, f, None), "cc_std")):
        assert lib.bmpc_dataset_moments_device(C.byref(_ds()), *args, None) == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("kw,word", [(dict(n=-1), "n must be"), (dict(n=1 << 31), "n must be"), (dict(goal_type=2), "goal_type"), (dict(index=None), "index"), (dict(x=None), "x"),
                                     (dict(y=None), "y"), (dict(states_mean=None), "states_mean"), (dict(states_std=None), "states_std"),
                                     (dict(goal_mean=None), "goal_mean"), (dict(goal_std=None), "goal_std")])
def test_batch_refusals_name_the_field(kw, word):
    rc = _lib_dataset.lib().bmpc_dataset_batch_device(C.byref(_ds()), C.byref(_batch(**kw)), None)
    assert rc == _lib.BAD_ARG and word in _lib.last_error(), _lib.last_error()


def test_batch_refuses_the_cc_mode_without_the_group():
    rc = _lib_dataset.lib().bmpc_dataset_batch_device(C.byref(_ds(w_cc=0, cc_goals=None)), C.byref(_batch()), None)
    assert rc == _lib.BAD_ARG and "goal_type cc" in _lib.last_error() and "without that group" in _lib.last_error()


# ---- the twin's ring: the reference's loop and dataset.Database ---------------------------------------------------------------------------

SIZES = (7, 30, 20, 0, 49, 120, 3)


def _loop_append(buf, start, length, limit, rows):
    """database.py:121-143, as tests/test_dataset_cpu.py restates it"""
    for r in rows:
        if length < limit:
            length += 1
        else:
            start = (start + 1) % limit
        buf[(start + length - 1) % limit] = r
    return start, length


def _groups(rng, shape, w_cc=12):
    return dict(states=rng.normal(size=shape + (43,)), actions=rng.normal(size=shape + (12,)), vc_goals=rng.normal(size=shape + (5,)),
                cc_goals=rng.normal(size=shape + (w_cc,)))


def _same(tw, db):
    return (tw.start, tw.length) == (db.start, db.length) and all(np.array_equal(tw.buf[k], getattr(db, k)) for k in twin.GROUPS)


def test_twin_ring_equals_the_loop_and_the_host_class():
    rng = np.random.default_rng(0)
    tw, db = twin.TwinDatabase(50), dataset.Database(50)
    ref, start, length = np.zeros((50, 43)), 0, 0
    for n in SIZES:
        g = _groups(rng, (n,))
        assert tw.append(**g) == n
        db.append(**g)
        start, length = _loop_append(ref, start, length, 50, g["states"])
        assert (tw.start, tw.length) == (start, length) and np.array_equal(tw.buf["states"], ref) and _same(tw, db)
    with pytest.raises(ValueError):
        tw.append(g["states"], g["actions"])


def test_twin_ring_with_rows_and_keep_dropping_problems():
    """(B, R) appends: the kept rows, b ascending then r ascending, equal Database.append of their concatenation"""
    rng = np.random.default_rng(1)
    tw, db = twin.TwinDatabase(50), dataset.Database(50)
    for B, R in ((3, 4), (5, 7), (4, 5), (2, 3), (7, 7), (12, 10), (1, 3)):
        g = _groups(rng, (B, R))
        rows, keep = rng.integers(-1, R + 2, size=B), (rng.random(B) > 0.3).astype(np.int32)
        n = tw.append(rows=rows, keep=keep, **g)
        sel = [(b, r) for b in range(B) if keep[b] for r in range(min(max(rows[b], 0), R))]
        assert n == len(sel)
        db.append(**{k: np.array([v[b, r] for b, r in sel]).reshape(len(sel), v.shape[2]) for k, v in g.items()})
        assert _same(tw, db)
    assert tw.length == 50 and tw.start != 0


def test_twin_ring_with_one_group_absent():
    rng = np.random.default_rng(2)
    for absent in ("vc_goals", "cc_goals"):
        tw, db = twin.TwinDatabase(50), dataset.Database(50)
        for i, n in enumerate(SIZES):
            g = _groups(rng, (n,))
            if i % 2:
                g.pop(absent)
            tw.append(**g)
            db.append(**g)
            assert _same(tw, db)
        assert np.any(tw.buf[absent] != 0)      # the slots of the absent group kept what was there


def test_twin_drops_a_problem_with_a_non_finite_kept_row():
    rng = np.random.default_rng(3)
    g = _groups(rng, (5, 4))
    rows = np.array([4, 3, 4, 2, 4])
    g["actions"][0, 3, 5] = np.nan          # the last kept row of problem 0
    g["cc_goals"][1, 0, 0] = np.inf         # problem 1
    g["states"][3, 2, 7] = np.nan           # beyond rows[3]: problem 3 stays
    tw = twin.TwinDatabase(50)
    assert tw.append(rows=rows, drop_nonfinite=True, **g) == 4 + 2 + 4
    assert np.array_equal(tw.buf["states"][:10], np.vstack([g["states"][2], g["states"][3, :2], g["states"][4]]))
    assert twin.TwinDatabase(50).append(rows=rows, **g) == 17


# ---- the twin's moments against exact arithmetic ------------------------------------------------------------------------------------------

def moment_data(rng, n):
    """(n, 43) and (n, 12): columns of scales 1e-3 .. 1e3 with offsets up to 1e3; states column 5 is the constant 0.1"""
    def cols(w):
        scale, offset = 10.0 ** rng.uniform(-3, 3, size=w), rng.uniform(-1e3, 1e3, size=w) * (rng.random(w) < 0.7)
        return rng.normal(size=(n, w)) * scale + offset
    s = cols(43)
    s[:, 5] = 0.1
    return s, cols(12)


@pytest.mark.parametrize("n", [1, 2, 3, 2000])
def test_twin_moments_against_exact_arithmetic(n):
    """numpy's mean and std, the twin's, within the bounds of tests/dataset_np.py::moment_violations of the exact values"""
    rng = np.random.default_rng(10 + n)
    s, c = moment_data(rng, n)
    tw = twin.TwinDatabase(max(n, 5))
    tw.append(s, rng.normal(size=(n, 12)), cc_goals=c)
    got = tw.moments()
    for k, a in (("states", s), ("cc_goals", c)):
        assert np.array_equal(got[k][0], np.mean(a, axis=0)) and np.array_equal(got[k][1], np.std(a, axis=0))
        assert twin.moment_violations(got[k][0], got[k][1], twin.exact_moments(a), n) == []
    assert got["states"][1][5] <= n * 2.0 ** -53 * 0.1
    with np.errstate(all="ignore"):
        empty = twin.TwinDatabase(5).moments()
    assert np.all(np.isnan(empty["states"][0])) and np.all(np.isnan(empty["states"][1]))


# ---- teeth: a twin with one fault fails the comparisons the GPU tests apply ---------------------------------------------------------------

def _sequence(fault):
    rng = np.random.default_rng(4)
    tw = twin.TwinDatabase(50, fault=fault)
    for B, R in ((3, 4), (5, 7), (4, 5), (7, 7), (1, 3)):
        tw.append(**_groups(rng, (B, R)))
    return tw


@pytest.mark.parametrize("fault", ["last_kept_row", "late_wrap"])
def test_a_faulty_ring_fails_the_bitwise_comparison(fault):
    good, bad = _sequence(None), _sequence(fault)
    assert not ((good.start, good.length) == (bad.start, bad.length) and all(np.array_equal(good.buf[k], bad.buf[k]) for k in twin.GROUPS))


def test_a_mean_over_limit_fails_the_moment_bounds():
    rng = np.random.default_rng(5)
    s, c = moment_data(rng, 30)
    bad = twin.TwinDatabase(50, fault="mean_over_limit")
    bad.append(s, rng.normal(size=(30, 12)), cc_goals=c)
    got = bad.moments()
    assert twin.moment_violations(got["states"][0], got["states"][1], twin.exact_moments(s), 30, factor=2) != []
