"""ctypes binding of include/bunmpc_foot_pairs.h (the switch and the telemetry of the headline kernel's force loop with two feet per
lane), read from that header at import with the reader of bunmpc.h (bunmpc_amd/_abi.py) and applied to the same libbunmpc_hip.so.  A
binding of its own, as bunmpc_amd/_lib_turn.py is: the table of bunmpc_amd._lib (tests/golden/abi.json) is the table of bunmpc.h alone."""
import os

from . import _abi, _lib
from . import build as _build

INCLUDE = os.path.join(os.path.dirname(_build.INCLUDE), "bunmpc_foot_pairs.h")
_ABI = _abi.read(INCLUDE, {})
_SIGS = _ABI.functions

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
        _applied = handle
    return handle
