"""Builds libbunmpc_hip.so (gfx950 kernels + C-ABI) in-tree with hipcc.

hipcc cross-compiles without a GPU; the built .so is git-ignored but travels with
the working tree to the GPU box.  compile_jobs() lists the objects; each is compiled on its own (cached under
csrc/_obj, keyed by the job's name and flags) and linked, so touching one source recompiles only its objects.

    python -m bunmpc_amd.build [--force] [--usage]
Environment: HIPCC, BUNMPC_EXTRA_FLAGS (extra compile flags, e.g. -DBWD_PROFILE), BUNMPC_LIB_OUT
(output path, for side-by-side experiment builds; load it with BUNMPC_LIB=<path>)."""
import concurrent.futures
import contextlib
import fcntl
import glob
import hashlib
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include", "bunmpc.h")
LIB = os.path.join(_HERE, "libbunmpc_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
# per-file extra flags (none now: -freciprocal-math -fapprox-func on ik_ddp.hip turns its 284 IEEE fp64 divisions into v_rcp_f64 +
# Newton steps, measured gain on the MI355X: none -- the divisions sit off the chains that set the pace -- so IEEE division stays)
# ik_ddp.hip: -ffp-contract=on.  hipcc's default for device code (fast) fuses a multiply into an add across statements, in the
# back end, where the decision depends on what surrounds the expression -- and the same source, instantiated once per wave role
# and per mapping, then rounds differently here and there (seen: one problem of 4096 whose final cost differed by one ulp between
# the four-problems-per-wave line search and the role-split one).  With `on` a product is fused only with the sum of its own
# expression, decided in the front end: every instantiation of a piece of source gets the same arithmetic, so "a problem's
# result does not depend on how it was scheduled" holds by construction.
# The fp32 centroidal units: no SLP vectoriser.  It packs pairs of fp32 operations into v_pk_mul/fma/add_f32, which need their operands
# in adjacent register pairs -- 47 v_mov_b32 per backtracking step to put them there, duplicated copies of the broadcast constants,
# 284-307 registers, and so 40-60 values spilled to scratch memory under the cap of 256 that two waves per SIMD need (345 MB of HBM
# traffic per launch against 75 MB of inputs and results; profiles/r02_pmc_hbm_cfg3.txt).  Without the packing the body takes 200-212
# registers: no scratch, and Go2 H = 40, B = 4096 goes 7.09 -> 6.02 ms.  (The fp64 kernels are ~0.5 % faster WITH the vectoriser, hence
# flags per unit.)  Their scratch bytes (AdmmUnit::scratch_bytes) being 0 is the point of -fno-slp-vectorize.
# -amdgpu-sched-strategy=max-ilp (the scheduler orders for instruction-level parallelism instead of register pressure): the
# one-problem-per-wave kernel is one long dependent chain per wave, batch-1 p50 1.49 -> 1.455 ms; the fp32 kernel 6.03 -> 5.97 ms.
# Timed and NOT taken elsewhere: the fp64 batch kernel (headline 4.095 -> 4.12 ms; its 64-lane shape 9.39 -> 9.24 ms) and ik_ddp.hip
# (derivative pass -2 %, Riccati pass and line search +1.5 %).
# -amdgpu-use-amdgpu-trackers (the scheduler follows register pressure with the target's own trackers): fp64 batch kernel, headline
# 4.095 -> 4.007 ms, its 64-lane shape 9.39 -> 8.95 ms; worse on ik_ddp.hip (Riccati pass +5 %) and on the one-problem-per-wave
# kernel (1.452 -> 1.469 ms), level on the fp32 kernel.  With it -amdgpu-disable-unclustered-high-rp-reschedule (no second scheduling
# pass against register pressure -- the kernel has 512 registers to itself): headline 4.014 -> 3.98 ms (64-lane shape 8.95 -> 9.0).
# No effect or worse on top: -amdgpu-schedule-metric-bias=0, -amdgpu-schedule-relaxed-occupancy, -amdgpu-early-ifcvt, max-ilp,
# -amdgpu-disable-clustered-low-occupancy-reschedule.
_FP64_ADMM_FLAGS = ["-mllvm", "-amdgpu-use-amdgpu-trackers", "-mllvm", "-amdgpu-disable-unclustered-high-rp-reschedule"]
_FP32_ADMM_FLAGS = ["-fno-slp-vectorize", "-mllvm", "-amdgpu-sched-strategy=max-ilp"]
# policy.hip: its fp32 results are held to a numpy twin in every bit, subnormal inputs, weights and sums included.  So, spelled out
# against whatever a toolchain's defaults or BUNMPC_EXTRA_FLAGS' neighbours may be: fp32 subnormals are kept (the matrix cores' A and
# B operands and the VALU honour the kernel's denormal mode), no fast-math (a NaN must stay a NaN through the ReLU, fmaf must stay one
# rounding), and no product is fused into a sum that the source does not fuse (fp64 normalisation, tau, err; the host packer's s and t).
# policy_train.hip (the training step) is held to its twin in the same way, operation by operation, and takes the same flags.
_POLICY_FLAGS = ["-fno-gpu-flush-denormals-to-zero", "-fno-fast-math", "-ffp-contract=off"]
# The centroidal units: biconvex_admm.hip compiled once per (cost shape, precision, feet), told which by three defines.  Every
# combination that a row of kShapes (biconvex_kernels.h) allows is listed here and nowhere else: biconvex_launch.hip's table refers to
# the accessor of each, so a library without one of them does not load.  A unit of its own per combination so that each is built with its
# own flags, the units build in parallel and one feature's kernels cannot disturb another's code object.  What the shapes are: kBlocks
# per-knot block-diagonal Q in set_cost_x / set_cost_f (the reference's ProblemData takes a sparse matrix, problem.cpp:31-56; a block
# per knot is the class that keeps the solve matrix-free with one knot per lane), kBand a block-tridiagonal Q with diagonal
# off-diagonal blocks (force-rate and momentum-rate terms D'R D), kCone the Euclidean projection onto the friction cone with per-foot
# coefficients (bmpc_cone_t; the reference's own "SoC" step, fista.cpp:52-70, is what every other unit restates), kConeFrame that
# cone about the contact's unit normal in place of world z (bmpc_contact_frame_t).
_FP64_SHAPES = ("kDiag", "kBlocks", "kBand", "kCone", "kConeFrame")
_FP32_SHAPES = ("kDiag",)


def compile_jobs():
    """[(name, source under csrc/, flags beside FLAGS)], one per object of the library, the longest compilations first (the fp64
    diagonal units: 44 kernels each) -- the only list of the library's sources, units, defines and per-object flags."""
    units = [(shape, precision, feet) for precision, shapes in ((0, _FP64_SHAPES), (1, _FP32_SHAPES)) for shape in shapes for feet in (4, 2)]
    jobs = [("admm_%s_%s_e%d" % (shape[1:].lower(), "f32" if precision else "f64", feet), "biconvex_admm.hip",
             ["-DADMM_UNIT_SHAPE=" + shape, "-DADMM_UNIT_PRECISION=%d" % precision, "-DADMM_UNIT_FEET=%d" % feet] +
             (_FP32_ADMM_FLAGS if precision else _FP64_ADMM_FLAGS)) for shape, precision, feet in units]
    # biconvex_launch.hip: host code and two helper kernels, which are held to the code the fp64 units' flags give them; lane_probe.hip: the
    # lane helpers of biconvex_lanes.h behind bmpc_probe_lanes, compiled as the fp64 units compile them; lie_probe.hip: the SE(3) primitives
    # of rbd_device.h behind bmpc_probe_lie, contracted as ik_ddp.hip contracts them
    others = {"biconvex_launch.hip": _FP64_ADMM_FLAGS, "lane_probe.hip": _FP64_ADMM_FLAGS, "biconvex_latency.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"], "bunmpc_capi.hip": [],
              "ik_ddp.hip": ["-ffp-contract=on"], "lie_probe.hip": ["-ffp-contract=on"], "bunmpc_ik_capi.hip": [], "plan_gen.hip": [], "id_ctrl.hip": [], "perturb.hip": [],
              "dataset.hip": [], "contact_log.hip": [], "policy.hip": _POLICY_FLAGS, "policy_train.hip": _POLICY_FLAGS, "acyclic_plan.hip": [], "cc_goals.hip": []}
    return jobs + [(src[:-len(".hip")], src, flags) for src, flags in others.items()]


def job(name):
    return next(j for j in compile_jobs() if j[0] == name)


def compile_cmd(job, extra_flags=()):
    """hipcc with the job's flags and source, without its output options"""
    return [HIPCC] + FLAGS + list(extra_flags) + job[2] + [os.path.join(CSRC, job[1])]


def object_path(job, flags):
    """... keyed by the job's name and its full flag list: two jobs of one source never share an object"""
    return os.path.join(OBJ, "%s.%s.o" % (job[0], hashlib.sha1(" ".join(list(flags) + job[2]).encode()).hexdigest()[:10]))


def dependencies():
    """every source of a job, every header of csrc/, the public header, every other header beside it (bunmpc_goals.h) or under ext/
    (bunmpc_acyclic.h) and this file (the flags live here)"""
    beside = sorted(h for h in glob.glob(os.path.join(os.path.dirname(INCLUDE), "*.h")) if h != INCLUDE)
    beside += sorted(glob.glob(os.path.join(os.path.dirname(INCLUDE), "ext", "*.h")))
    return (sorted({os.path.join(CSRC, src) for _, src, _ in compile_jobs()}) + sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [INCLUDE] + beside +
            [os.path.abspath(__file__)])


def _without_mllvm(cmd):
    out, skip = [], False
    for tok in cmd:
        if skip:
            skip = False
        elif tok == "-mllvm":
            skip = True
        else:
            out.append(tok)
    return out


def is_stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in dependencies())


@contextlib.contextmanager
def build_lock():
    """One builder at a time per tree (the ranks of a multi-GPU job start together and share csrc/_obj and the .so): the
    first to arrive builds, the others wait here and then find the library fresh."""
    os.makedirs(OBJ, exist_ok=True)
    with open(os.path.join(OBJ, ".build.lock"), "w") as f:
        fcntl.flock(f, fcntl.LOCK_EX)
        try:
            yield
        finally:
            fcntl.flock(f, fcntl.LOCK_UN)


def build(force=False, verbose=False, extra_flags=()):
    out = os.environ.get("BUNMPC_LIB_OUT", LIB)
    if not force and out == LIB and not is_stale():
        return LIB
    with build_lock():
        if not force and out == LIB and not is_stale():      # another process built it while this one waited
            return LIB
        return _build_locked(out, force, verbose, extra_flags)


def _compile(cmd):
    if subprocess.call(cmd) != 0:
        # -mllvm options are LLVM-internal switches (scheduler tuning worth 1-3 %), not a stable interface: another hipcc may not
        # know them ("Unknown command line argument").  One retry without them; -ffp-contract=on and -fno-slp-vectorize stay --
        # they carry the bit-identity and no-scratch guarantees (tests/test_biconvex_gpu.py, tests/test_ik_gpu.py).
        plain = _without_mllvm(cmd)
        if plain == cmd:
            raise subprocess.CalledProcessError(1, cmd)
        print("bunmpc_amd.build: retrying without -mllvm options: " + " ".join(plain), file=sys.stderr)
        subprocess.check_call(plain)


def _build_locked(out, force, verbose, extra_flags):
    if not os.path.exists(HIPCC):
        raise RuntimeError("hipcc not found at %s: cannot build %s" % (HIPCC, out))
    extra = os.environ.get("BUNMPC_EXTRA_FLAGS", "").split() + list(extra_flags)
    os.makedirs(OBJ, exist_ok=True)
    newest_header = max(os.path.getmtime(d) for d in dependencies() if d.endswith(".h"))
    objs, cmds = [], []
    for j in compile_jobs():
        op = object_path(j, FLAGS + extra)
        objs.append(op)
        if force or not os.path.exists(op) or os.path.getmtime(op) < max(os.path.getmtime(os.path.join(CSRC, j[1])), newest_header):
            cmds.append(compile_cmd(j, extra) + ["-c", "-o", op])
            if verbose:
                print(" ".join(cmds[-1]), file=sys.stderr)
    with concurrent.futures.ThreadPoolExecutor(max_workers=16) as pool:      # at most 16 compilers at a time, started in the jobs' order
        list(pool.map(_compile, cmds))
    tmp = "%s.tmp.%d" % (out, os.getpid())     # linked beside, then renamed: a process loading the library never sees half of it
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    os.replace(tmp, out)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True,
                extra_flags=["-Rpass-analysis=kernel-resource-usage"] if "--usage" in sys.argv else []))
