"""ctypes binding of libbunmpc_hip.so.  Signatures, structs and constants are read from every header of include/ at import
(bunmpc_amd/_abi.py): the headers are the one declaration of the C-ABI, and this module is their one binding.  A new header gets a row
in HEADER_NAMES below and nothing else.  There is no CPU fallback: if the library is missing and cannot be built, or a call needs a GPU that
is not there, this raises."""
import contextlib
import ctypes as C
import os
import re

from . import _abi
from . import build as _build

# every header of include/, in a fixed order, with the Python name of every struct it declares; a header without a row here and a struct
# without a name are errors, not omissions
HEADER_NAMES = {
    "bunmpc.h": {
        "bmpc_batch_t": "Batch", "bmpc_launch_plan_t": "LaunchPlan", "bmpc_block_cost_t": "BlockCost", "bmpc_band_cost_t": "BandCost",
        "bmpc_cone_t": "Cone", "bmpc_contact_frame_t": "ContactFrame", "bmpc_ik_sched_t": "IkSched", "bmpc_ik_batch_t": "IkBatch",
        "bmpc_ik_planned_launch_t": "IkPlannedLaunch", "bmpc_ik_iter_plan_t": "IkIterPlan", "bmpc_kinodyn_batch_t": "KinoDynBatch",
        "bmpc_gait_params_t": "GaitParams", "bmpc_plan_batch_t": "PlanBatch", "bmpc_wb_plan_batch_t": "WbPlanBatch",
        "bmpc_terrain_t": "Terrain", "bmpc_interp_batch_t": "InterpBatch", "bmpc_id_batch_t": "IdBatch", "bmpc_perturb_batch_t": "PerturbBatch",
    },
    "bunmpc_goals.h": {"bmpc_cc_gait_t": "CcGait", "bmpc_cc_goal_batch_t": "CcGoalBatch", "bmpc_cc_goal_wb_batch_t": "CcGoalWbBatch"},
    "bunmpc_turn.h": {"bmpc_turn_t": "Turn"},
    "bunmpc_foot_pairs.h": {},
}


def read_headers(include, names):
    """{file name: Abi} of the headers of directory `include`, in the order of the table `names`.  ImportError, with the header and the
    names in it, where the directory and the table list different headers, a header's structs differ from its rows, two headers declare
    one function, struct or class name, or two headers give one #define different values."""
    found = {f for f in os.listdir(include) if f.endswith(".h")}
    if found != set(names):
        raise ImportError("include/ and the header table of bunmpc_amd/_lib.py differ in " + ", ".join(sorted(found ^ set(names))))
    headers, owner, values = {}, {}, {}
    for header, rows in names.items():
        abi = _abi.read(os.path.join(include, header), rows)
        if set(abi.structs) != set(rows):
            raise ImportError("include/%s and its name table in bunmpc_amd/_lib.py differ in %s" % (header, ", ".join(sorted(set(abi.structs) ^ set(rows)))))
        for kind, declared in (("function", abi.functions), ("struct", abi.structs), ("class name", rows.values())):
            twice = sorted(n for n in declared if owner.setdefault((kind, n), header) != header)
            if twice:
                raise ImportError("include/%s declares the %s %s again, after include/%s" % (header, kind, ", ".join(twice), owner[kind, twice[0]]))
        for name, value in abi.defines.items():
            first, old = values.setdefault(name, (header, value))
            if old != value:
                raise ImportError("#define %s is %r in include/%s and %r in include/%s" % (name, old, first, value, header))
        headers[header] = abi
    return headers


HEADERS = read_headers(os.path.dirname(_build.INCLUDE), HEADER_NAMES)
_NAMES = {c: py for rows in HEADER_NAMES.values() for c, py in rows.items()}      # the union, like _ABI: no name is declared twice
_ABI = _abi.Abi(*({k: v for abi in HEADERS.values() for k, v in getattr(abi, part).items()} for part in _abi.Abi._fields))      # the union
globals().update((cls.__name__, cls) for cls in _ABI.structs.values())      # Batch, Cone, Turn, ...: the ctypes classes, docstring = C name

_SIGS = _ABI.functions      # {name: (restype, [argtypes])}
OK, BAD_ARG, DIVERGED, DEVICE_ERROR = (_ABI.defines["BMPC_" + n] for n in ("OK", "BAD_ARG", "DIVERGED", "DEVICE_ERROR"))
L0_X, L0_F = _ABI.defines["BMPC_L0_X"], _ABI.defines["BMPC_L0_F"]
IK_NODE_TASK_DOUBLES = _ABI.defines["BMPC_IK_NODE_TASK_DOUBLES"]
NSTATS = 6

# the dispatch knobs, {keyword: setter}: a process default whose setter takes the new value and returns the old one.  bmpc_set_<name> is
# knob <name>, bmpc_ik_set_<name> is knob ik_<name>; bmpc_set_device has the shape and returns a status
_NOT_KNOBS = {"bmpc_set_device"}
KNOBS = {(m.group(1) or "") + m.group(2): f for f, (res, args) in _SIGS.items()
         if (m := re.fullmatch(r"bmpc_(ik_)?set_(\w+)", f)) and args == [res] and f not in _NOT_KNOBS}

_lib = None


class BmpcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bunmpc status %d: %s" % (code, msg))
        self.code = code


def exported_symbols():
    """Every symbol the headers of include/ declare (checked by the CPU tests)."""
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
        for header, abi in HEADERS.items():
            for name, (res, args) in abi.functions.items():
                fn = getattr(handle, name)  # AttributeError if the library lacks a declared symbol
                fn.restype = res
                fn.argtypes = args
            for cname, cls in abi.structs.items():      # bmpc_<stem>_t against bmpc_<stem>_struct_size(), where the header declares one
                size = cname[:-len("_t")] + "_struct_size"
                if size in abi.functions and getattr(handle, size)() != C.sizeof(cls):
                    raise ImportError("%s layout differs between include/%s and bunmpc_amd/_lib.py" % (cname, header))
        _lib = handle
    return _lib


def check(code):
    if code != OK:
        raise BmpcError(code, lib().bmpc_last_error().decode())
    return code


def last_error():
    return lib().bmpc_last_error().decode()


@contextlib.contextmanager
def knobs(**values):
    """Process defaults set for the block through their setters (KNOBS), in the order given, and put back in reverse order after it,
    also when the block raises: with knobs(two_waves_per_simd=1, ik_express=0): ..."""
    unknown = sorted(set(values) - set(KNOBS))
    if unknown:
        raise TypeError("knobs() got an unknown knob: " + ", ".join(unknown))
    handle, old = lib(), []
    try:
        for k, v in values.items():
            old.append((KNOBS[k], getattr(handle, KNOBS[k])(v)))
        yield
    finally:
        for setter, v in reversed(old):
            getattr(handle, setter)(v)
