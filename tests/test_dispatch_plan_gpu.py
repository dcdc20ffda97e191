"""The pure dispatch function against what is actually launched (run with -m gpu): a sample of tests/golden/dispatch_table.json is
solved again, and the "last launch" record must equal both the table (recorded on an MI355X before the launch layer was folded) and
bmpc_biconvex_plan_launch given this device's SIMD count.  And the per-device state of the launch layer on a second GPU, if there is one."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from bunmpc_amd import _lib
from tests import dispatch_rows as dr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launches_are_what_the_plan_and_the_table_say(hiplib):
    import torch
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    table_simds, rows = dr.load()
    # every seventh row, and every row of the kernels and switches that are rare in the table
    sample = [r for i, r in enumerate(rows) if i % 7 == 0 or r["kernel"] in ("refused", "biconvex_admm_steal_kernel") or r["knob"] == "steal_grid"]
    assert len(sample) >= 100
    wrong = []
    for row in sample:
        got = dr.solve(row)
        out, d = _lib.LaunchPlan(), dr.descriptor(row)
        with dr.knob(hiplib, row["knob"], row["value"]):
            rc = hiplib.bmpc_biconvex_plan_launch(C.byref(d), dr.SHAPES[row["shape"]], simds, C.byref(out))
        if row["kernel"] == "refused":
            ok = got[0] == "refused" and rc != 0
        else:
            planned = (out.kernel.decode(), out.lanes_per_problem, out.waves_per_simd or None)
            ok = rc == 0 and got == planned and (simds != table_simds or got == (row["kernel"], row["lanes"], row["waves"]))
        if not ok:
            wrong.append((row, got, rc, out.kernel, out.lanes_per_problem, out.waves_per_simd))
    assert not wrong, "%d of %d rows differ, the first: %s" % (len(wrong), len(sample), wrong[:5])


_SECOND_DEVICE = r"""
import ctypes as C, hashlib, sys
import numpy as np
import torch
from bunmpc_amd import _lib, batch as bb, problems
lib = _lib.lib()
b = problems.make_batch("solo12_trot", 3, H=219)
nx, nf = 9 * 220, 12 * 219
rng = np.random.default_rng(5)
raw = dict(Qx=rng.uniform(1.0, 10.0, (3, nx)), qx=rng.standard_normal((3, nx)), lbx=np.full((3, nx), -1e3), ubx=np.full((3, nx), 1e3),
           Qf=rng.uniform(1e-4, 1e-3, (3, nf)))
digests = []
for dev in (0, 1):
    _lib.check(lib.bmpc_set_device(dev))
    torch.cuda.set_device(dev)
    d = bb.DeviceBatch(b, device="cuda:%d" % dev, num_iters=2, raw=raw)
    d.solve()
    out = d.results()
    assert lib.bmpc_biconvex_last_kernel_name() == b"biconvex_admm_wg_kernel" and lib.bmpc_biconvex_last_lanes_per_problem() == 256
    digests.append(hashlib.sha256(b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("X", "F", "P", "L_x", "L_f", "stats"))).hexdigest())
assert digests[0] == digests[1], digests
print("SECOND_DEVICE_OK")
"""


def test_second_device_gets_its_own_launch_state(hiplib):
    """220 knots in the raw form: the workgroup kernel with more than 64 KB of LDS, whose raised limit -- like the momentum table and the
    SIMD count -- is kept per device.  A fresh child process solves the batch on device 0, switches with bmpc_set_device(1) and solves
    it again with its buffers there: both succeed, byte-identical."""
    n = C.c_int(0)
    _lib.check(hiplib.bmpc_device_count(C.byref(n)))
    if n.value < 2:
        pytest.skip("one GPU: the per-device launch state needs two")
    p = subprocess.run([sys.executable, "-c", _SECOND_DEVICE], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "SECOND_DEVICE_OK" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
