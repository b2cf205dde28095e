"""ctypes binding of the test / tuning companion library (include/qqq_amd_dev.h, libqqq_amd_dev.so).

Used by tests/, bench.py and tools/ only -- the operator (qqq_amd.ops, qqq_amd.qlinear) never imports this module."""
from __future__ import annotations

import ctypes
import os

from . import _abi, _lib
from . import build as _build

_dev = None


def lib():
    global _dev
    if _dev is not None:
        return _dev
    _lib.lib()  # the operator library (and the HIP runtime torch brought in) first
    path = _build.DEV_LIB
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python qqq_amd/build.py` (needs hipcc)")
    L = ctypes.CDLL(path)
    _abi.bind(L, _build.header("qqq_amd_dev.h"))
    _dev = L
    return L


def gemm_ex_ptr(operator_lib=None):
    """address of qqq_w4a8_gemm_ex in the operator library (what qqq_dev_bench_gemm times)"""
    L = operator_lib if operator_lib is not None else _lib.lib()
    return ctypes.cast(L.qqq_w4a8_gemm_ex, ctypes.c_void_p)


def gemm_ex2_ptr(operator_lib=None):
    """address of qqq_w4a8_gemm_ex2 (what qqq_dev_bench_gemm2 times)"""
    L = operator_lib if operator_lib is not None else _lib.lib()
    return ctypes.cast(L.qqq_w4a8_gemm_ex2, ctypes.c_void_p)


def last_error() -> str:
    return lib().qqq_dev_last_error().decode()
