"""ctypes binding of the C-ABI in include/qqq_amd*.h and include_ops/qqq_amd*.h, bound from the headers' own prototypes (qqq_amd/_abi.py).  No fallback: if the HIP
library is missing or does not load, every entry point raises -- the product path never routes through a CPU implementation."""
from __future__ import annotations

import ctypes
import os

from . import _abi
from . import build as _build

_lib = None
ABI_VERSION = _abi.define(_build.header("qqq_amd.h"), "QQQ_AMD_ABI_VERSION")
QQQTune = _abi.QQQTune  # struct qqq_tune, field for field


def lib():
    global _lib
    if _lib is not None:
        return _lib
    # torch first: it brings the HIP runtime (SONAME libamdhip64.so.7) into the process, and our
    # library's NEEDED entry then binds to that same runtime (one HIP runtime per process).
    import torch  # noqa: F401

    path = _build.LIB
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the gfx950 HIP kernels are not built. Run `python -c 'import "
            "__graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback."
        )
    L = ctypes.CDLL(path)
    if L.qqq_amd_abi_version() != ABI_VERSION:  # (int(void): callable before it is bound; a stale library may lack what the headers declare)
        raise RuntimeError("libqqq_amd.so ABI version mismatch; rebuild")
    for hdr in _build.operator_headers() + _build.operator_op_headers():
        _abi.bind(L, hdr)
    _lib = L
    return L


def last_error() -> str:
    return lib().qqq_amd_last_error().decode()


def plan(m, n, k, groupsize=-1, max_par=16, have_scratch=True, have_workspace=True, tune=None) -> dict:
    """the dispatch decision for one problem (host logic only, no GPU work): see qqq_w4a8_plan"""
    tn = None
    if tune:
        tn = QQQTune()
        for key, v in tune.items():
            setattr(tn, key, int(v))
    out = QQQTune()
    rc = lib().qqq_w4a8_plan(m, n, k, groupsize, max_par, int(have_scratch), int(have_workspace),
                             ctypes.byref(tn) if tn is not None else None, ctypes.byref(out))
    if rc:
        raise RuntimeError(f"qqq_w4a8_plan failed ({rc}): {last_error()}")
    return {f: getattr(out, f) for f, _ in QQQTune._fields_}


def model_us(m, n, k, groupsize=-1, max_par=16) -> dict:
    """the cost models' price (us) of each family for one problem: {"column", "stream", "panel", "wide"} (families that are no candidate are left out)"""
    out = (ctypes.c_double * 4)()
    rc = lib().qqq_w4a8_model_us(m, n, k, groupsize, max_par, out)
    if rc:
        raise RuntimeError(f"qqq_w4a8_model_us failed ({rc}): {last_error()}")
    return {name: out[i] for i, name in enumerate(("column", "stream", "panel", "wide")) if out[i] > 0}
