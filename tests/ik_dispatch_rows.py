"""Solves of tests/golden/ik_dispatch_table.json: what every host look of an IK-DDP batch solve launched.

A solve is (name, B, n_col, has_list, knobs, sched): `knobs` are process defaults set through the bmpc_ik_set_* calls (KNOB_SETTERS),
`sched` the fields of the batch's own bmpc_ik_sched_t.  tools/record_ik_dispatch.py runs each in a fresh process under a kernel trace
and writes, per solve,
  fused_direct, fused_grid       the whole batch went through one launch of ik_fused_kernel (and its workgroups)
  select_launches                launches of ik_select_kernel (the express lane's look, iterations 2..12 until it has taken its problems)
  express_launches, express_grid launches of ik_fused_kernel on the side stream, and their workgroups
  iters_run, last_calcdiff       what the solve reported (bmpc_ik_batch_t.iters_run, bmpc_ik_last_calcdiff_kernel)
  looks                          one row per chunk of iterations between two ik_publish_active_kernel launches:
                                 [first iteration, active, chunk, state, derivative, Riccati, line search], each kernel as
                                 [name, workgroups, workgroup size]; active is the Riccati kernel's grid, or null without an active list
                                 (every launch covers all B problems then) after the second chunk (the first two are enqueued before the
                                 host's first look: active = B)
The CPU test asks bmpc_ik_plan_iteration the same questions; the GPU test solves a few of them again (run())."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ik_dispatch_table.json")
MAXITER = 40
KNOB_SETTERS = {"spec_below": "speculative_below", "spec_one_wave_above": "spec_one_wave_above", "all_steps": "all_steps",
                "gains_wave_below": "gains_wave_below", "calcdiff_one_wave_above": "calcdiff_one_wave_above", "express_cap": "express_capacity",
                "fused_direct": "fused_direct_max"}
DEFAULTS = {"spec_below": 1024, "spec_one_wave_above": 0, "all_steps": 0, "gains_wave_below": 512, "calcdiff_one_wave_above": 1024,
            "express_cap": 96, "fused_direct": 16}
SCHED_FIELDS = ("spec_below", "all_steps_below", "gains_wave_below", "express_cap", "debug_inject")


def solves():
    """(name, B, n_col, has_list, knobs, sched)"""
    small = dict(spec_below=24, all_steps=4, gains_wave_below=12, spec_one_wave_above=16)
    return [
        # B = 48, five running nodes: the thresholds among the active counts the batch passes through ...
        ("b48_small_knobs", 48, 5, 1, dict(small, calcdiff_one_wave_above=40), {}),
        ("b48_small_knobs_calcdiff_100", 48, 5, 1, dict(small, calcdiff_one_wave_above=100), {}),
        # ... and each line-search mapping at the first look
        ("b48_two_waves", 48, 5, 1, dict(calcdiff_one_wave_above=143), dict(spec_below=48, gains_wave_below=-1)),
        ("b48_one_wave", 48, 5, 1, dict(spec_below=100, spec_one_wave_above=16, calcdiff_one_wave_above=144), {}),
        ("b48_three_waves", 48, 5, 1, {}, dict(spec_below=200)),
        ("b48_all_steps", 48, 5, 1, dict(all_steps=9), dict(all_steps_below=64, spec_below=-1)),
        ("b48_defaults", 48, 5, 1, {}, {}),
        ("b48_no_list", 48, 5, 0, dict(small, calcdiff_one_wave_above=40), {}),
        # the fused kernel: a whole small batch in one launch, or not
        ("b16_fused_direct", 16, 5, 1, {}, {}),
        ("b16_loop", 16, 5, 1, dict(fused_direct=0), {}),
        ("b17_above_fused_direct", 17, 5, 1, {}, {}),
        ("b16_no_list", 16, 5, 0, {}, {}),
        # the express lane
        ("b64_express_forced", 64, 5, 1, {}, dict(debug_inject=2)),
        ("b64_express_forced_cap_4", 64, 5, 1, dict(express_cap=4), dict(debug_inject=2)),
        ("b64_express_off", 64, 5, 1, {}, dict(express_cap=-1, debug_inject=2)),
        ("b64_defaults", 64, 5, 1, {}, {}),
        ("b63_below_express", 63, 5, 1, {}, dict(debug_inject=2)),
        # geometry: one node pair; three nodes (an odd tail pair); a part-filled wave of the four-per-wave line search; odd pair counts
        ("b5_one_node_pair", 5, 1, 1, dict(fused_direct=0, spec_below=0, calcdiff_one_wave_above=1), {}),
        ("b5_one_node_pair_two_waves", 5, 1, 1, dict(fused_direct=0, spec_below=3), {}),
        ("b5_three_nodes", 5, 2, 1, dict(fused_direct=0, spec_below=0, calcdiff_one_wave_above=1), {}),
        ("b5_three_nodes_fused", 5, 2, 1, {}, {}),
        ("b1_one_node_pair", 1, 1, 1, dict(fused_direct=-1), {}),
        # 65 nodes: more than the fused kernel holds, fused-direct and the express lane are refused
        ("b5_long_horizon", 5, 64, 1, {}, {}),
        ("b64_long_horizon", 64, 64, 1, {}, dict(debug_inject=2)),
    ]


def by_name(name):
    return next(s for s in solves() if s[0] == name)


def load():
    with open(TABLE) as f:
        return json.load(f)["solves"]


def knobs(values):
    """process defaults set for the block, restored after it: bunmpc_amd._lib.knobs by the short keys of the table"""
    from bunmpc_amd import _lib
    return _lib.knobs(**{"ik_" + KNOB_SETTERS[k]: v for k, v in values.items()})


def sched_of(fields):
    from bunmpc_amd import _lib
    s = _lib.IkSched()
    for k, v in fields.items():
        assert k in SCHED_FIELDS
        setattr(s, k, v)
    return s


@functools.lru_cache(maxsize=1)
def _base():
    from bunmpc_amd import problems, urdf_model
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model = urdf_model.RobotModel.from_json(open(os.path.join(root, "bunmpc_amd", "robots", "solo12.json")).read())
    return model, problems.make_wb_batch(model, 64)


class IkDeviceBatch:
    """B Solo12 trot IK problems of n_col running nodes on the device: the nodes of problems.make_wb_batch's task list, cut or repeated
    to n_col (the momentum task tracks zero: no centroidal solve runs here)"""

    def __init__(self, B, n_col, has_list, sched=None, device="cuda"):
        import torch
        from bunmpc_amd import _lib
        from bunmpc_amd.inverse_kinematics_cpp import as_device_model
        model, wb = _base()
        self.torch, self.device, self.B, self.T = torch, torch.device(device), B, n_col
        self.dm = as_device_model(model)
        node = np.arange(n_col) % wb.ik_T
        tasks = np.concatenate([wb.ik_tasks[:B, node], wb.ik_tasks[:B, -1:]], axis=1)
        dt = wb.dyn.dt[:B, node]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)       # noqa: E731
        self.arr = dict(x0=up(wb.x[:B]), dt=up(dt), tasks=up(tasks), state_w=up(wb.state_w), x_reg=up(wb.x_reg[:B]), ctrl_w=up(wb.ctrl_w))
        lib = _lib.lib()
        self.ws = torch.zeros((B, lib.bmpc_ik_workspace_doubles(n_col)), dtype=torch.float64, device=self.device)
        self.active = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.active_list = torch.zeros(lib.bmpc_ik_active_list_ints(B), dtype=torch.int32, device=self.device)
        self.iters_run = C.c_int(0)
        d = _lib.IkBatch()
        d.B, d.n_col, d.maxiter, d.model = B, n_col, MAXITER, self.dm.h
        for k, v in self.arr.items():
            setattr(d, k, v.data_ptr())
        d.ws, d.active, d.iters_run = self.ws.data_ptr(), self.active.data_ptr(), C.addressof(self.iters_run)
        d.active_list = self.active_list.data_ptr() if has_list else None
        for k, v in (sched or {}).items():
            assert k in SCHED_FIELDS
            setattr(d.sched, k, v)
        self.desc = d

    def solve(self):
        """one batch solve; returns (iters_run, which derivative kernel ran last, sha256 of the solutions xs | us and the scalars)"""
        from bunmpc_amd import _lib
        lib = _lib.lib()
        self.ws.zero_()
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(lib.bmpc_ik_solve_batch_device(C.byref(self.desc), C.c_void_p(stream)))
        self.torch.cuda.synchronize(self.device)
        last = lib.bmpc_ik_last_calcdiff_kernel()
        off = (C.c_long * 8)()
        lib.bmpc_ik_layout(self.T, off)
        ws = self.ws.cpu().numpy()
        h = hashlib.sha256()
        for o, n in ((off[0], (self.T + 1) * 37), (off[1], self.T * 18)):
            h.update(np.ascontiguousarray(ws[:, o:o + n]).tobytes())
        h.update(np.ascontiguousarray(ws[:, [off[2] + i for i in (0, 4, 8, 10)]]).tobytes())      # cost, stopping criterion, iterations, status
        return self.iters_run.value, last, h.hexdigest()


def run(solve):
    """the solve under its knobs: (iters_run, last derivative kernel, digest)"""
    name, B, n_col, has_list, knob_values, sched = solve
    with knobs(knob_values):
        return IkDeviceBatch(B, n_col, has_list, sched).solve()
