"""Binding of include/ext/bunmpc_policy_train.h (the policy network's training step and its packed image on the device), in the pattern of
bunmpc_amd/_lib_policy.py: the header is read with bunmpc_amd/_abi.py and its signatures are applied to the handle of bunmpc_amd._lib.lib()
at first use, where the three struct sizes are checked against the library's."""
import ctypes as C
import os

from . import _abi, _lib
from . import build as _build

HEADER = os.path.join(os.path.dirname(_build.INCLUDE), "ext", "bunmpc_policy_train.h")
NAMES = {"bmpc_policy_params_t": "PolicyParams", "bmpc_policy_train_t": "PolicyTrain", "bmpc_policy_step_t": "PolicyStep"}
ABI = _abi.read(HEADER, NAMES)
if set(ABI.structs) != set(NAMES):
    raise ImportError("include/ext/bunmpc_policy_train.h and its name table in bunmpc_amd/_lib_policy_train.py differ in " + ", ".join(sorted(set(ABI.structs) ^ set(NAMES))))
PolicyParams, PolicyTrain, PolicyStep = (ABI.structs[n] for n in ("bmpc_policy_params_t", "bmpc_policy_train_t", "bmpc_policy_step_t"))
MAX_ROWS, PAD = ABI.defines["BMPC_POLICY_TRAIN_MAX_ROWS"], ABI.defines["BMPC_POLICY_TRAIN_PAD"]

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
                raise ImportError("%s layout differs between include/ext/bunmpc_policy_train.h and the library" % cname)
        _bound = handle
    return _bound
