"""ctypes binding of include/bunmpc_turn.h (turning commands through the device-side plan builders), read from that header at import
with the reader of bunmpc.h (bunmpc_amd/_abi.py) and applied to the same libbunmpc_hip.so.  Its struct class lives here and not in
bunmpc_amd._lib, whose table (tests/golden/abi.json) is the table of bunmpc.h alone; tests/golden/abi_turn.json is this one's."""
import ctypes as C
import math
import os

from . import _abi, _lib
from . import build as _build

INCLUDE = os.path.join(os.path.dirname(_build.INCLUDE), "bunmpc_turn.h")
# the Python name of every struct of the header; a struct without a row here is an error, not an omission
_NAMES = {"bmpc_turn_t": "Turn"}
_ABI = _abi.read(INCLUDE, _NAMES)
if set(_ABI.structs) != set(_NAMES):
    raise ImportError("include/bunmpc_turn.h and the name table of bunmpc_amd/_lib_turn.py differ in " + ", ".join(sorted(set(_ABI.structs) ^ set(_NAMES))))
globals().update((_NAMES[c], cls) for c, cls in _ABI.structs.items())

_SIGS = _ABI.functions
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
                raise ImportError("%s layout differs between include/bunmpc_turn.h and bunmpc_amd/_lib_turn.py" % cname)
        _applied = handle
    return handle


def turn_struct(yaw_inertia, w_des=None):
    """bmpc_turn_t; w_des: a device tensor (B,) of float64 (the whole-body call) or None (the centroidal-level call).  A yaw inertia
    the C calls would refuse raises here, where the caller's argument has a name."""
    yaw_inertia = float(yaw_inertia)
    if not (math.isfinite(yaw_inertia) and yaw_inertia > 0.0):
        raise ValueError("yaw_inertia must be finite and > 0, got %r" % (yaw_inertia,))
    t = Turn()      # noqa: F821 (from the header)
    t.w_des, t.yaw_inertia = None if w_des is None else w_des.data_ptr(), yaw_inertia
    return t
