"""Rows of tests/golden/dispatch_table.json: which centroidal kernel a batch of a given shape gets.

A row is (E, k, B, form, precision, num_iters, shape, knob, value, kernel, lanes, waves):
  E, k, B         feet, knots (H + 1), problems
  form            "harness", "raw" or "raw_qf" (raw with a linear force cost)
  precision       0 fp64, 1 fp32
  shape           "diag", "blocks" or "band"
  knob, value     one dispatch switch away from its default (the name of its bmpc_set_* call without that prefix), or null
  kernel          what bmpc_biconvex_last_kernel_name reported after the solve, or "refused" where the call returned an error
  lanes, waves    bmpc_biconvex_last_lanes_per_problem / _last_waves_per_simd; waves is null after the one-problem-per-wave kernel,
                  which leaves that record as the launch before it set it

tools/record_dispatch.py fills the last three columns by solving every row of cases() on the GPU; the CPU test asks
bmpc_biconvex_plan_launch the same questions (descriptor() + knob()), the GPU test solves a sample of them again (solve())."""
import contextlib
import ctypes as C
import dataclasses
import functools
import json
import os

import numpy as np

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatch_table.json")
COLUMNS = ("E", "k", "B", "form", "precision", "num_iters", "shape", "knob", "value", "kernel", "lanes", "waves")
SHAPES = {"diag": 0, "blocks": 1, "band": 2}
K_ALL = (2, 16, 17, 21, 22, 32, 33, 64, 65, 127, 128, 129, 192, 193, 209, 256)
K_SEG = K_ALL[:8]            # one problem per wave segment
B_ALL = (1, 1024, 1025, 3072, 4096, 6144)
KNOBS = (("three_per_wave", 0), ("three_per_wave", 1), ("two_waves_per_simd", 0), ("two_waves_per_simd", 1), ("work_stealing", 0),
         ("latency_mapping_max_batch", 0), ("steal_grid", 512))


def cases():
    """(E, k, B, form, precision, num_iters, shape, knob, value) of every row, combinations that cannot differ left out"""
    out = []

    def add(E, k, B, form="harness", precision=0, iters=10, shape="diag", knob=None, value=0):
        out.append((E, k, B, form, precision, iters, shape, knob, value))
    for k in K_ALL:                                     # defaults, harness form, fp64
        for B in B_ALL:
            add(4, k, B)
        for B in (1, 4096):
            add(2, k, B)
    for iters in (25, 100):                             # the ADMM iteration count: three per wave, work stealing
        for k in (16, 17, 21, 22, 64, 65):
            for B in B_ALL:
                add(4, k, B, iters=iters)
        for B in (3072, 4096, 6144):
            add(2, 21, B, iters=iters)
    for form in ("raw", "raw_qf"):
        for k in (2, 17, 21, 33, 65, 129, 209, 256):
            for B in (1, 1025, 4096):
                add(4, k, B, form)
        add(4, 21, 6144, form, iters=100)
        add(2, 209, 1025, form)
    for k in K_SEG:                                     # fp32: harness form, at most 64 knots
        for B in (1, 1024, 1025, 4096):
            add(4, k, B, precision=1)
    add(2, 17, 4096, precision=1)
    add(2, 64, 4096, precision=1)
    for shape in ("blocks", "band"):
        for k in K_SEG:
            for B in (1, 1024, 3072, 4096, 6144):
                add(4, k, B, "raw", shape=shape)
        for k in (17, 21):
            for B in (1, 4096):
                add(4, k, B, "raw_qf", iters=25, shape=shape)
        add(2, 21, 3072, "raw", shape=shape)
        add(2, 64, 3072, "raw", shape=shape)
        for value in (0, 1):
            add(4, 21, 4096, "raw", shape=shape, knob="three_per_wave", value=value)
    for knob, value in KNOBS:
        for k in (16, 21, 32, 64, 65, 129, 209):
            for B in (1, 1025, 4096):
                add(4, k, B, knob=knob, value=value)
        for B in (1, 4096, 6144):
            add(4, 21, B, iters=100, knob=knob, value=value)
    # what the library refuses
    add(4, 21, 4, "raw", precision=1)
    add(4, 21, 4, "raw", precision=1, shape="blocks")
    add(4, 21, 4, "raw", precision=1, shape="band")
    add(4, 21, 4, "harness", shape="blocks")
    add(4, 21, 4, "harness", shape="band")
    add(4, 65, 4, "raw", shape="blocks")
    add(4, 65, 4, "raw", shape="band")
    add(4, 65, 4, precision=1)
    add(4, 257, 4)
    add(4, 257, 4, "raw")
    add(3, 21, 4)
    add(3, 21, 4, "raw")
    assert len(set(out)) == len(out)
    return out


def load():
    with open(TABLE) as f:
        t = json.load(f)
    assert tuple(t["columns"]) == COLUMNS
    return t["simds"], [dict(zip(COLUMNS, r)) for r in t["rows"]]


@contextlib.contextmanager
def knob(lib, name, value):
    """one dispatch switch set for the block (name None: none), restored after it"""
    if name is None:
        yield
        return
    fn = getattr(lib, "bmpc_set_" + name)
    old = fn(value)
    try:
        yield
    finally:
        fn(old)


def descriptor(row):
    """the scalar fields of the row's bmpc_batch_t (weights shared by the batch: strides 0); every pointer null"""
    from bunmpc_amd import _lib
    d = _lib.Batch()
    _lib.lib().bmpc_batch_defaults(C.byref(d))
    d.B, d.n_col, d.n_eff = row["B"], row["k"] - 1, row["E"]
    d.raw = 0 if row["form"] == "harness" else 1
    d.precision, d.num_iters, d.cold_start = row["precision"], row["num_iters"], 1
    return d


def last_launch(lib):
    return lib.bmpc_biconvex_last_kernel_name().decode(), lib.bmpc_biconvex_last_lanes_per_problem(), lib.bmpc_biconvex_last_waves_per_simd()


def solve(row):
    """Solve a batch of the row's shape through batch.solve_host (B copies of one problem, one FISTA iteration per phase: the dispatch
    reads sizes only) and return the (kernel, lanes, waves) record it leaves, or ("refused", None, None)"""
    from bunmpc_amd import _lib, batch
    E, k, B, H = row["E"], row["k"], row["B"], row["k"] - 1
    b = _copies("biped_walk" if E == 2 else "solo12_trot", B, H)
    if E == 3:      # (no such batch exists: the sizes of one, for the call to refuse)
        b = dataclasses.replace(b, E=3, cnt_plan=b.cnt_plan[:, :, :3], W_F=np.ones((1, 9 * H)))
    raw = None
    if row["form"] != "harness":
        nx, nf = 9 * k, 3 * E * H
        raw = dict(Qx=np.ones((B, nx)), qx=np.zeros((B, nx)), lbx=np.full((B, nx), -1e3), ubx=np.full((B, nx), 1e3), Qf=np.full((B, nf), 1e-4))
        if row["form"] == "raw_qf":
            raw["qf"] = np.full((B, nf), 1e-6)
    if row["shape"] == "blocks":
        raw = {} if raw is None else raw
        raw.update(Qx_blk=np.tile(np.eye(9), (1, k, 1, 1)), Qf_blk=np.tile(1e-4 * np.eye(3 * E), (1, H, 1, 1)))
    if row["shape"] == "band":
        raw = {} if raw is None else raw
        raw.update(Qx_off=np.zeros((1, H, 9)), Qf_off=np.zeros((1, H - 1, 3 * E)))
    lib = _lib.lib()
    with knob(lib, row["knob"], row["value"]):
        try:
            if row["form"] == "harness" and raw is not None:      # (block / band arrays with the harness form: straight to the C call)
                _harness_with_cost(lib, b, row, raw)
            else:
                batch.solve_host(b, num_iters=row["num_iters"], maxit=1, raw=raw, precision="f32" if row["precision"] else "f64")
        except _lib.BmpcError:
            return "refused", None, None
        name, lanes, waves = last_launch(lib)
    return name, lanes, (None if name == "biconvex_latency_kernel" else waves)


@functools.lru_cache(maxsize=2)
def _copies(config, B, H):
    """B copies of the config's first problem, weights shared by the batch"""
    from bunmpc_amd import problems
    b = problems.make_batch(config, 1, H=H).take(np.zeros(B, dtype=np.int64))
    return dataclasses.replace(b, W_X=b.W_X[:1], W_X_ter=b.W_X_ter[:1], W_F=b.W_F[:1], bounds=b.bounds[:1])


def _harness_with_cost(lib, b, row, raw):
    """bmpc_biconvex_solve_batch_blocks_host / _band_host with a harness-form descriptor (batch.solve_host has no such call)"""
    from bunmpc_amd import _lib
    d = descriptor(row)
    if row["shape"] == "blocks":
        c = _lib.BlockCost(Qx_blk=raw["Qx_blk"].ctypes.data, Qf_blk=raw["Qf_blk"].ctypes.data)
        _lib.check(lib.bmpc_biconvex_solve_batch_blocks_host(C.byref(d), C.byref(c)))
    else:
        c = _lib.BandCost(Qx_off=raw["Qx_off"].ctypes.data, Qf_off=raw["Qf_off"].ctypes.data)
        _lib.check(lib.bmpc_biconvex_solve_batch_band_host(C.byref(d), C.byref(c)))
