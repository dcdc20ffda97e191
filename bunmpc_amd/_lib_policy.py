"""Binding of include/ext/bunmpc_policy.h (the policy network's forward pass on the device): the header is read with the reader of every
other (bunmpc_amd/_abi.py) and its signatures are applied to the handle of bunmpc_amd._lib.lib() at first use, where the three struct
sizes are checked against the library's.  Headers under include/ext/ are bound by a module of their own; the table of bunmpc_amd._lib
lists the headers directly in include/."""
import ctypes as C
import os

from . import _abi, _lib
from . import build as _build

HEADER = os.path.join(os.path.dirname(_build.INCLUDE), "ext", "bunmpc_policy.h")
NAMES = {"bmpc_policy_net_t": "PolicyNetDesc", "bmpc_policy_weights_t": "PolicyWeights", "bmpc_policy_rows_t": "PolicyRows"}
ABI = _abi.read(HEADER, NAMES)
if set(ABI.structs) != set(NAMES):
    raise ImportError("include/ext/bunmpc_policy.h and its name table in bunmpc_amd/_lib_policy.py differ in " + ", ".join(sorted(set(ABI.structs) ^ set(NAMES))))
PolicyNetDesc, PolicyWeights, PolicyRows = (ABI.structs[n] for n in ("bmpc_policy_net_t", "bmpc_policy_weights_t", "bmpc_policy_rows_t"))
STATE_WIDTH, Q_WIDTH, V_WIDTH, TAU_WIDTH = (ABI.defines["BMPC_POLICY_" + n] for n in ("STATE_WIDTH", "Q_WIDTH", "V_WIDTH", "TAU_WIDTH"))
MAX_LAYERS, MAX_WIDTH, MAX_OUT, PAD = (ABI.defines["BMPC_POLICY_" + n] for n in ("MAX_LAYERS", "MAX_WIDTH", "MAX_OUT", "PAD"))
ACTION_TYPE = {"torque": ABI.defines["BMPC_POLICY_TORQUE"], "pd_target": ABI.defines["BMPC_POLICY_PD_TARGET"],
               "structured": ABI.defines["BMPC_POLICY_STRUCTURED"]}

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
                raise ImportError("%s layout differs between include/ext/bunmpc_policy.h and the library" % cname)
        _bound = handle
    return _bound
