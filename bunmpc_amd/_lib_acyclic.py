"""Binding of include/ext/bunmpc_acyclic.h (acyclic motions on the device): the header is read with the reader of every other
(bunmpc_amd/_abi.py) and its signatures are applied to the handle of bunmpc_amd._lib.lib() at first use, where the two struct sizes are
checked against the library's.  Headers under include/ext/ are bound by a module of their own; the table of bunmpc_amd._lib lists
the headers directly in include/."""
import ctypes as C
import os

from . import _abi, _lib
from . import build as _build

HEADER = os.path.join(os.path.dirname(_build.INCLUDE), "ext", "bunmpc_acyclic.h")
NAMES = {"bmpc_acyclic_plan_t": "AcyclicPlan", "bmpc_hold_batch_t": "HoldBatch"}
ABI = _abi.read(HEADER, NAMES)
if set(ABI.structs) != set(NAMES):
    raise ImportError("include/ext/bunmpc_acyclic.h and its name table in bunmpc_amd/_lib_acyclic.py differ in " + ", ".join(sorted(set(ABI.structs) ^ set(NAMES))))
AcyclicPlan, HoldBatch = ABI.structs["bmpc_acyclic_plan_t"], ABI.structs["bmpc_hold_batch_t"]
FRAME_SLOTS, MAX_PHASES = ABI.defines["BMPC_ACY_FRAME_SLOTS"], ABI.defines["BMPC_ACY_MAX_PHASES"]

_bound = None


def lib():
    """the library's handle with this header's signatures applied"""
    global _bound
    if _bound is None:
        handle = _lib.lib()
        for name, (res, args) in ABI.functions.items():
            fn = getattr(handle, name)      # AttributeError if the library lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        for cname, cls in ABI.structs.items():
            if getattr(handle, cname[:-len("_t")] + "_struct_size")() != C.sizeof(cls):
                raise ImportError("%s layout differs between include/ext/bunmpc_acyclic.h and the library" % cname)
        _bound = handle
    return _bound
