"""ctypes binding of libbunmpc_hip.so.  Signatures, structs and constants are read from include/bunmpc.h at import
(bunmpc_amd/_abi.py): the header is the one declaration of the C-ABI.  There is no CPU fallback: if the library is missing and
cannot be built, or a call needs a GPU that is not there, this raises."""
import ctypes as C
import os

from . import _abi
from . import build as _build

# the Python name of every struct of the header; a struct without a row here is an error, not an omission
_NAMES = {
    "bmpc_batch_t": "Batch", "bmpc_launch_plan_t": "LaunchPlan", "bmpc_block_cost_t": "BlockCost", "bmpc_band_cost_t": "BandCost",
    "bmpc_cone_t": "Cone", "bmpc_contact_frame_t": "ContactFrame", "bmpc_ik_sched_t": "IkSched", "bmpc_ik_batch_t": "IkBatch",
    "bmpc_ik_planned_launch_t": "IkPlannedLaunch", "bmpc_ik_iter_plan_t": "IkIterPlan", "bmpc_kinodyn_batch_t": "KinoDynBatch",
    "bmpc_gait_params_t": "GaitParams", "bmpc_plan_batch_t": "PlanBatch", "bmpc_wb_plan_batch_t": "WbPlanBatch",
    "bmpc_terrain_t": "Terrain", "bmpc_interp_batch_t": "InterpBatch", "bmpc_id_batch_t": "IdBatch", "bmpc_perturb_batch_t": "PerturbBatch",
}
_ABI = _abi.read(_build.INCLUDE, _NAMES)
if set(_ABI.structs) != set(_NAMES):
    raise ImportError("include/bunmpc.h and the name table of bunmpc_amd/_lib.py differ in " + ", ".join(sorted(set(_ABI.structs) ^ set(_NAMES))))
globals().update((_NAMES[c], cls) for c, cls in _ABI.structs.items())      # Batch, Cone, ...: the ctypes classes, docstring = C name

_SIGS = _ABI.functions      # {name: (restype, [argtypes])}
OK, BAD_ARG, DIVERGED, DEVICE_ERROR = (_ABI.defines["BMPC_" + n] for n in ("OK", "BAD_ARG", "DIVERGED", "DEVICE_ERROR"))
L0_X, L0_F = _ABI.defines["BMPC_L0_X"], _ABI.defines["BMPC_L0_F"]
IK_NODE_TASK_DOUBLES = _ABI.defines["BMPC_IK_NODE_TASK_DOUBLES"]
NSTATS = 6

_lib = None


class BmpcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bunmpc status %d: %s" % (code, msg))
        self.code = code


def exported_symbols():
    """Every symbol include/bunmpc.h declares (checked by the CPU tests)."""
    return sorted(_SIGS)


def _preload_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's).  Two HIP
    runtimes in one process do not work (the second sees no device), so when torch is installed
    bind this library to torch's copy whichever of the two is imported first."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    global _lib
    if _lib is None:
        _preload_hip_runtime()
        path = os.environ.get("BUNMPC_LIB")     # side-by-side experiment builds (bunmpc_amd/build.py)
        if not path:
            path = _build.LIB
            if not os.path.exists(path) or (_build.is_stale() and os.path.exists(_build.HIPCC)):
                path = _build.build()
        handle = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(handle, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        for cname, cls in _ABI.structs.items():      # bmpc_<stem>_t against bmpc_<stem>_struct_size(), where the header declares one
            size = cname[:-len("_t")] + "_struct_size"
            if size in _SIGS and getattr(handle, size)() != C.sizeof(cls):
                raise ImportError("%s layout differs between include/bunmpc.h and bunmpc_amd/_lib.py" % cname)
        _lib = handle
    return _lib


def check(code):
    if code != OK:
        raise BmpcError(code, lib().bmpc_last_error().decode())
    return code


def last_error():
    return lib().bmpc_last_error().decode()
