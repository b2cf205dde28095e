"""ctypes binding of libqqq_amd_quant.so, bound from the prototypes of every header in qqq_amd/quant/include/, qqq_amd/quant/include_ext/
and qqq_amd/quant/include_ops/ (build.quant_headers(), build.quant_ext_headers(), build.quant_op_headers(), qqq_amd/_abi.py).  No fallback: if the library is missing, every entry point raises."""
from __future__ import annotations

import ctypes
import os

from .. import _abi
from .. import build as _build

_lib = None
HEADER = _build.QUANT_HEADER
ABI_VERSION = _abi.define(HEADER, "QQQ_AMD_QUANT_ABI_VERSION")
ERR_ARG = _abi.define(_build.header("qqq_amd.h"), "QQQ_ERR_ARG")


def lib():
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (torch first: one HIP runtime per process, as qqq_amd/_lib.py)

    path = _build.QUANT_LIB
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the gfx950 quantiser kernels are not built. Run `python -c 'import "
            "__graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback."
        )
    L = ctypes.CDLL(path)
    if L.qqq_quant_abi_version() != ABI_VERSION:
        raise RuntimeError("libqqq_amd_quant.so ABI version mismatch; rebuild")
    for hdr in _build.quant_headers() + _build.quant_ext_headers() + _build.quant_op_headers():
        _abi.bind(L, hdr)
    _lib = L
    return L


def last_error() -> str:
    return lib().qqq_quant_last_error().decode()
