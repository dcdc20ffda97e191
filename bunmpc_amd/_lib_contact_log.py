"""Binding of include/ext/bunmpc_contact_log.h (measured contact goals: contact logs to cc_goals rows on the device): the header is
read with the reader of every other (bunmpc_amd/_abi.py) and its signatures are applied to the handle of bunmpc_amd._lib.lib() at first
use, where the struct size is checked against the library's.  Headers under include/ext/ are bound by a module of their own; the table
of bunmpc_amd._lib lists the headers directly in include/."""
import ctypes as C
import os

from . import _abi, _lib
from . import build as _build

HEADER = os.path.join(os.path.dirname(_build.INCLUDE), "ext", "bunmpc_contact_log.h")
NAMES = {"bmpc_contact_log_t": "ContactLog"}
ABI = _abi.read(HEADER, NAMES)
if set(ABI.structs) != set(NAMES):
    raise ImportError("include/ext/bunmpc_contact_log.h and its name table in bunmpc_amd/_lib_contact_log.py differ in " + ", ".join(sorted(set(ABI.structs) ^ set(NAMES))))
ContactLog = ABI.structs["bmpc_contact_log_t"]
FEW_SWITCHES, START_AFTER_END, PAST_SCHEDULE, EVENTS_OVERFLOW, FAILED_STATE = (
    ABI.defines["BMPC_CL_" + n] for n in ("FEW_SWITCHES", "START_AFTER_END", "PAST_SCHEDULE", "EVENTS_OVERFLOW", "FAILED_STATE"))

_bound = None


def lib():
    """the library's handle with this header's signatures applied"""
    global _bound
    if _bound is None:
        handle = _lib.lib()
        for name, (res, args) in ABI.functions.items():
            fn = getattr(handle, name)      # AttributeError if the library lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        if handle.bmpc_contact_log_struct_size() != C.sizeof(ContactLog):
            raise ImportError("bmpc_contact_log_t layout differs between include/ext/bunmpc_contact_log.h and the library")
        _bound = handle
    return _bound
