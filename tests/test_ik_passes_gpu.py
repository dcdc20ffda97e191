"""GPU tests of the IK-DDP kernels PASS BY PASS (ik_ddp.hip through bmpc_ik_selftest_passes): one derivative pass and one Riccati
pass at a trajectory of the test's choosing, the workspace read back and
  * every node of the derivative pass (cost, xnext, F_x, F_u, L_x, L_xx, L_u, diag L_uu, the gaps, the summed cost) compared with
    the two CPU twins at the same (x, u), within max(10 x the twins' own gap on that case, the bound the twins are held to);
  * the Riccati pass (K, k, d1, d2, the stopping criterion, the final regularisation and feasibility flag) compared with the
    long-double Riccati reference fed with the kernel's OWN unpacked derivatives, within 10 x the distance of the float64 run of that
    reference from the long-double run on the same inputs;
  * both derivative kernels (two waves / one wave per node pair) and both Riccati mappings (with / without the gains wave) bit for
    bit against each other, at pass level and over a whole solve.
References, cases and tolerances: tests/ik_passes_np.py, pinned by tests/test_ik_passes_cpu.py."""
import ctypes as C
import time

import numpy as np
import pytest

from bunmpc_amd import _lib, problems
from tests import ik_passes_np as P

pytestmark = pytest.mark.gpu
NV, NDX, NX = P.NV, P.NDX, P.NX
COMBOS = ((0, 1), (1, 1), (0, 2), (1, 2))        # (derivative kernel: 0 two waves per pair, 1 one wave; waves of the Riccati pass)
# Floors under the Riccati yardstick, from the number format alone (u = 2^-53): where the float64 run happens to round to within a
# fraction of an ulp of the long-double result, 10 x that distance is below what ANY other order of the same fp64 operations can
# meet.  K, k: a 36-term product and an 18-step elimination per entry, (36 + 18) u; d1, d2, stop: sums of 18 T same-signed terms,
# (18 T) u -- the classical bound on reordering a sum (Higham, Accuracy and Stability, (4.4)).
U = 2.0 ** -53


def riccati_floor(q, T):
    return (36 + 18) * U if q in ("K", "k") else 18 * T * U


class PassBatch:
    """device copies of a case + its bmpc_ik_batch_t"""

    def __init__(self, case, device="cuda"):
        import torch
        from bunmpc_amd.inverse_kinematics_cpp import as_device_model
        self.torch, self.case, self.device = torch, case, torch.device(device)
        self.dm = as_device_model(case.model)
        B, T = case.B, case.T
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)       # noqa: E731
        self.arr = {k: up(getattr(case, k)) for k in ("x0", "dt", "tasks", "state_w", "x_reg", "ctrl_w", "xs", "us")}
        assert case.ctrl_w.shape[-2:] == (T, NV) or case.weights != "node"        # no terminal row: [n_col][18] as include/bunmpc.h says
        lib = _lib.lib()
        self.lay = P.layout(T)
        assert self.lay["total"] == lib.bmpc_ik_workspace_doubles(T)
        self.ws = torch.zeros((B, self.lay["total"]), dtype=torch.float64, device=self.device)
        self.active = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.active_list = torch.zeros(lib.bmpc_ik_active_list_ints(B), dtype=torch.int32, device=self.device)
        d = _lib.IkBatch()
        d.B, d.n_col, d.maxiter, d.model = B, T, 1, self.dm.h
        for k in ("x0", "dt", "tasks", "state_w", "x_reg", "ctrl_w"):
            setattr(d, k, self.arr[k].data_ptr())
        per_b = case.state_w.shape[0] != 1
        if case.weights == "node":
            d.s_state_w, d.sn_state_w = (T + 1) * NDX, NDX
            d.s_x_reg, d.sn_x_reg = (T + 1) * NX, NX
            d.s_ctrl_w, d.sn_ctrl_w = T * NV, NV
        else:
            d.s_state_w, d.s_ctrl_w = (NDX, NV) if per_b else (0, 0)
        d.ws, d.active, d.active_list = self.ws.data_ptr(), self.active.data_ptr(), self.active_list.data_ptr()
        self.desc = d

    def run(self, calcdiff_kernel, bwd_waves, feasible=None, xreg=None):
        """one derivative pass + one Riccati pass; returns the workspace [B][total] (host copy)"""
        self.ws.zero_()
        self.torch.cuda.synchronize(self.device)
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        lib = _lib.lib()
        _lib.check(lib.bmpc_ik_selftest_passes(C.byref(self.desc), C.c_void_p(self.arr["xs"].data_ptr()), C.c_void_p(self.arr["us"].data_ptr()),
                                               self.case.feasible if feasible is None else feasible,
                                               self.case.xreg if xreg is None else xreg, calcdiff_kernel, bwd_waves, C.c_void_p(stream)))
        assert lib.bmpc_ik_last_calcdiff_kernel() == calcdiff_kernel          # which derivative kernel the launch was
        return self.ws.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def riccati_block(ws, lay, T):
    """K, k and the scalars of every problem: what the two Riccati mappings must agree on bit for bit"""
    return np.concatenate([ws[:, lay["K"]:lay["K"] + T * NV * NDX], ws[:, lay["kff"]:lay["kff"] + T * NV], ws[:, lay["scal"]:lay["scal"] + 16]], axis=1)


CASES = {c.name: c for c in P.cases("all")}
RATIOS = {}          # case -> quantity -> error / bound (printed; EXPERIMENTS.md holds the table of a run)


@pytest.mark.parametrize("name", list(CASES))
def test_passes_against_the_references(name):
    case = CASES[name]
    B, T = case.B, case.T
    t0 = time.time()
    pb = PassBatch(case)
    lay = pb.lay
    runs = {combo: pb.run(*combo) for combo in COMBOS}
    t_gpu = time.time() - t0
    # ---- kernel variants: same bits
    ws = runs[(0, 1)]
    assert same_bits(ws, runs[(1, 1)]), "the two derivative kernels differ (one Riccati wave)"
    assert same_bits(runs[(0, 2)], runs[(1, 2)]), "the two derivative kernels differ (with the gains wave)"
    assert same_bits(riccati_block(ws, lay, T), riccati_block(runs[(0, 2)], lay, T)), "the two Riccati mappings differ"
    # ---- derivative pass against the twins
    tw = P.twins_on_case(case)
    dt = case.dt
    got = [[dict(P.unpack_node(ws[b], lay, t, dt[b, min(t, T - 1)], T), cost=ws[b, lay["node_cost"] + t]) for t in range(T + 1)] for b in range(B)]
    fs_got = ws[:, lay["fs"]:lay["fs"] + (T + 1) * NDX].reshape(B, T + 1, NDX)
    worst = P.deriv_errors(case, got, fs_got, tw)
    ratios = {q: worst[q][0] / tw["tol"][q] for q in P.DERIV_QUANTITIES}
    sc = ws[:, lay["scal"]:lay["scal"] + 16]
    cost_err = 0.0
    for b in range(B):
        own = 0.0
        for t in range(T + 1):
            own += got[b][t]["cost"]
        assert sc[b, P.SCAL["cost"]] == own, "S_COST is not the sum of the node costs in node order"
        ref_sum, ref_abs = 0.0, 0.0
        for t in range(T + 1):
            ref_sum += tw["c"][b][t]["cost"]
            ref_abs += abs(tw["c"][b][t]["cost"])
        cost_err = max(cost_err, abs(sc[b, P.SCAL["cost"]] - ref_sum) / ref_abs)
    ratios["S_COST"] = cost_err / tw["tol"]["cost"]
    # ---- Riccati pass against the long-double reference on the kernel's own derivatives
    feas_want = 1.0 if case.feasible or not np.any(np.abs(tw["fs_c"]) >= 1e-16) else 0.0
    ric = {q: 0.0 for q in P.RICCATI_QUANTITIES}
    on_floor = {q: 0 for q in P.RICCATI_QUANTITIES}      # comparisons that 10 x the float64 distance alone would have failed
    retries = []
    for b in range(B):
        data = [{k: v for k, v in got[b][t].items() if k in ("Lx", "Lxx", "Lu", "Luu", "Fx", "Fu")} for t in range(T + 1)]
        ref, f64, bound = P.riccati_bounds(data, fs_got[b], case.xreg, case.feasible)
        assert not ref["gave_up"] and ref["retries"] == f64["retries"], (b, ref["retries"], f64["retries"])
        retries.append(ref["retries"])
        assert sc[b, P.SCAL["xreg"]] == f64["reg"], (b, sc[b, P.SCAL["xreg"]], f64["reg"])        # as many retries as the reference's rule
        assert sc[b, P.SCAL["feas"]] == feas_want and sc[b, P.SCAL["status"]] == 0.0 and sc[b, P.SCAL["done"]] == 0.0
        gpu = dict(K=ws[b, lay["K"]:lay["K"] + T * NV * NDX].reshape(T, NV, NDX), k=ws[b, lay["kff"]:lay["kff"] + T * NV].reshape(T, NV),
                   d1=sc[b, P.SCAL["d1"]], d2=sc[b, P.SCAL["d2"]], stop=sc[b, P.SCAL["stop"]])
        err = P.riccati_errors(gpu, ref)
        for q in P.RICCATI_QUANTITIES:
            bq = max(bound[q], riccati_floor(q, T))
            on_floor[q] += int(bound[q] < riccati_floor(q, T) and err[q] > bound[q])
            ric[q] = max(ric[q], err[q] / bq)
    ratios.update(ric)
    RATIOS[name] = ratios
    print("\nPASSES %-40s %s | retries %s | decided by the fp64 floor: %s | gpu %.1fs total %.1fs"
          % (name, "  ".join("%s %.2g" % kv for kv in ratios.items()), sorted(set(retries)), " ".join("%s %d" % kv for kv in on_floor.items()), t_gpu, time.time() - t0))
    if case.indefinite:
        assert min(retries) >= 3, retries           # Q_uu was indefinite until the regularisation had grown: the retry path ran
    over = {q: r for q, r in ratios.items() if not r <= 1.0}
    assert not over, (name, over, {q: worst[q] for q in over if q in worst})


def test_selftest_arguments_are_checked():
    case = CASES["solo12_T1_a0_shared"]
    pb = PassBatch(case)
    lib = _lib.lib()
    xs, us = C.c_void_p(pb.arr["xs"].data_ptr()), C.c_void_p(pb.arr["us"].data_ptr())
    for args in ((None, us, 0, 1e-9, 0, 1), (xs, None, 0, 1e-9, 0, 1), (xs, us, 2, 1e-9, 0, 1), (xs, us, 0, 0.0, 0, 1), (xs, us, 0, float("nan"), 0, 1),
                 (xs, us, 0, 1e-9, 2, 1), (xs, us, 0, 1e-9, 0, 3), (xs, us, 0, 1e-9, 0, 0)):
        assert lib.bmpc_ik_selftest_passes(C.byref(pb.desc), *args, None) == _lib.BAD_ARG, args
    assert lib.bmpc_ik_selftest_passes(None, xs, us, 0, 1e-9, 0, 1, None) == _lib.BAD_ARG
    off = (C.c_long * 8)()
    assert lib.bmpc_ik_layout_all(case.T, off, 8) == len(P.LAYOUT_KEYS)
    old = (C.c_long * 8)()
    lib.bmpc_ik_layout(case.T, old)
    assert list(off) == list(old)


def test_whole_solve_does_not_depend_on_the_derivative_kernel():
    """one Solo12 whole-body batch solved with every derivative launch on the one-wave kernel, then with every launch on the two-wave
    kernel (the lock-step path: no fused kernel): every output bit for bit; and the DDP loop's own choice by launch size"""
    from bunmpc_amd.kinodyn_batch import KinoDynDeviceBatch
    lib = _lib.lib()
    model = P.load_model("solo12")
    wb = problems.make_wb_batch(model, 6)
    out, ran = [], []
    old_fd = lib.bmpc_ik_set_fused_direct_max(0)
    old = lib.bmpc_ik_set_calcdiff_one_wave_above(0)
    try:
        assert old == 1024
        for above in (0, 1 << 30):
            lib.bmpc_ik_set_calcdiff_one_wave_above(above)
            kb = KinoDynDeviceBatch(wb, model, num_iters=10)
            kb.solve()
            out.append(kb.results())
            ran.append(lib.bmpc_ik_last_calcdiff_kernel())
        # the default bound: a launch of 256 x 6 = 1536 node pairs takes the one-wave kernel, one of 5 x 6 the two-wave kernel
        lib.bmpc_ik_set_calcdiff_one_wave_above(old)
        for name, want in (("solo12_B256_T10_a0.5_shared", 1), ("solo12_T10_a0.5_node_vel10", 0)):
            pb = PassBatch(CASES[name])
            stream = pb.torch.cuda.current_stream(pb.device).cuda_stream
            _lib.check(lib.bmpc_ik_solve_batch_device(C.byref(pb.desc), C.c_void_p(stream)))        # maxiter = 1: one derivative launch over all B
            assert lib.bmpc_ik_last_calcdiff_kernel() == want, name
    finally:
        lib.bmpc_ik_set_calcdiff_one_wave_above(old)
        lib.bmpc_ik_set_fused_direct_max(old_fd)
    assert ran == [1, 0]
    a, b = out
    assert np.all(a["ik_status"] == 0) and a["ik_iters"].min() > 1
    for k in ("xs", "us", "ik_cost", "ik_stop", "ik_iters", "ik_status"):
        assert np.array_equal(a[k], b[k]), k
    n = a["ik_iters"]
    for i in range(len(n)):
        assert np.array_equal(a["ik_trace"][i, :n[i]], b["ik_trace"][i, :n[i]]), i
