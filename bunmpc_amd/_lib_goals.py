"""ctypes binding of include/bunmpc_goals.h (contact-conditioned goals), read from that header at import with the reader of
bunmpc.h (bunmpc_amd/_abi.py) and applied to the same libbunmpc_hip.so.  Its struct classes live here and not in bunmpc_amd._lib, whose
table (tests/golden/abi.json) is the table of bunmpc.h alone."""
import ctypes as C
import os

from . import _abi, _lib
from . import build as _build

INCLUDE = os.path.join(os.path.dirname(_build.INCLUDE), "bunmpc_goals.h")
# the Python name of every struct of the header; a struct without a row here is an error, not an omission
_NAMES = {"bmpc_cc_gait_t": "CcGait", "bmpc_cc_goal_batch_t": "CcGoalBatch", "bmpc_cc_goal_wb_batch_t": "CcGoalWbBatch"}
_ABI = _abi.read(INCLUDE, _NAMES)
if set(_ABI.structs) != set(_NAMES):
    raise ImportError("include/bunmpc_goals.h and the name table of bunmpc_amd/_lib_goals.py differ in " + ", ".join(sorted(set(_ABI.structs) ^ set(_NAMES))))
globals().update((_NAMES[c], cls) for c, cls in _ABI.structs.items())

_SIGS = _ABI.functions
FEW_SWITCHES, START_AFTER_END, PAST_SCHEDULE, EVENTS_OVERFLOW = (
    _ABI.defines["BMPC_CC_" + n] for n in ("FEW_SWITCHES", "START_AFTER_END", "PAST_SCHEDULE", "EVENTS_OVERFLOW"))
check, BmpcError, BAD_ARG = _lib.check, _lib.BmpcError, _lib.BAD_ARG

_applied = None


def exported_symbols():
    return sorted(_SIGS)


def lib():
    """the library of bunmpc_amd._lib with this header's signatures on it"""
    global _applied
    handle = _lib.lib()
    if _applied is not handle:
        for name, (res, args) in _SIGS.items():
            fn = getattr(handle, name)      # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        for cname, cls in _ABI.structs.items():
            size = cname[:-len("_t")] + "_struct_size"
            if size in _SIGS and getattr(handle, size)() != C.sizeof(cls):
                raise ImportError("%s layout differs between include/bunmpc_goals.h and bunmpc_amd/_lib_goals.py" % cname)
        _applied = handle
    return handle


def gait_struct(gait):
    g = CcGait()      # noqa: F821 (from the header)
    g.gait_period, g.gait_dt, g.gait_horizon = gait.gait_period, gait.gait_dt, gait.gait_horizon
    for j in range(4):
        g.stance_percent[j], g.phase_offset[j] = gait.stance_percent[j], gait.phase_offset[j]
    return g


def plan_knots(episode_length, gait, sim_dt=0.001):
    """H_cp of contact_planner.py:130, through the C-ABI (no GPU)"""
    return lib().bmpc_cc_goal_plan_knots(int(episode_length), float(sim_dt), float(gait.gait_horizon), float(gait.gait_period), float(gait.gait_dt))
