"""Binding of include/ext/bunmpc_dataset.h (the trainers' data set on the device): the header is read with the reader of every other
(bunmpc_amd/_abi.py) and its signatures are applied to the handle of bunmpc_amd._lib.lib() at first use, where the three struct sizes
are checked against the library's.  Headers under include/ext/ are bound by a module of their own; the table of bunmpc_amd._lib lists
the headers directly in include/."""
import ctypes as C
import os

from . import _abi, _lib
from . import build as _build

HEADER = os.path.join(os.path.dirname(_build.INCLUDE), "ext", "bunmpc_dataset.h")
NAMES = {"bmpc_dataset_t": "Dataset", "bmpc_dataset_rows_t": "DatasetRows", "bmpc_dataset_batch_t": "DatasetBatch"}
ABI = _abi.read(HEADER, NAMES)
if set(ABI.structs) != set(NAMES):
    raise ImportError("include/ext/bunmpc_dataset.h and its name table in bunmpc_amd/_lib_dataset.py differ in " + ", ".join(sorted(set(ABI.structs) ^ set(NAMES))))
Dataset, DatasetRows, DatasetBatch = (ABI.structs[n] for n in ("bmpc_dataset_t", "bmpc_dataset_rows_t", "bmpc_dataset_batch_t"))
STATE_WIDTH, VC_WIDTH, ACTION_WIDTH = ABI.defines["BMPC_DS_STATE_WIDTH"], ABI.defines["BMPC_DS_VC_WIDTH"], ABI.defines["BMPC_DS_ACTION_WIDTH"]
MAX_CC_WIDTH, MAX_PROBLEMS, HEADER_LONGS = ABI.defines["BMPC_DS_MAX_CC_WIDTH"], ABI.defines["BMPC_DS_MAX_PROBLEMS"], ABI.defines["BMPC_DS_HEADER_LONGS"]
GOAL = {"vc": ABI.defines["BMPC_DS_GOAL_VC"], "cc": ABI.defines["BMPC_DS_GOAL_CC"]}

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
                raise ImportError("%s layout differs between include/ext/bunmpc_dataset.h and the library" % cname)
        _bound = handle
    return _bound
