"""The Cholesky factor op without a GPU: its header binds beside the others, the workspace size is host arithmetic, and the entry
point refuses bad arguments before anything touches a device."""
import ctypes
import os


def test_factor_header_binds_and_sizes_the_workspace():
    from qqq_amd import _abi, build
    from qqq_amd.quant import _lib as qlib

    L = qlib.lib()
    header = os.path.join(build.QUANT_INCLUDE, "qqq_amd_factor.h")
    assert header in build.quant_headers() and set(_abi.prototypes(header)) == {"qqq_upper_factor_work", "qqq_upper_factor"}
    assert len(L.qqq_upper_factor.argtypes) == 9 and L.qqq_quant_abi_version() == 1
    nbytes = ctypes.c_longlong(0)
    for n in (64, 192, 11008, 32768):
        assert L.qqq_upper_factor_work(n, ctypes.byref(nbytes)) == 0 and nbytes.value == 4 * (n * n + 128 * n)
    for n in (0, 96, 32832):
        assert L.qqq_upper_factor_work(n, ctypes.byref(nbytes)) == qlib.ERR_ARG and qlib.last_error().startswith("qqq_upper_factor_work: n=")
    assert L.qqq_upper_factor(None, 64, None, 64, 64, None, None, 0, None) == qlib.ERR_ARG
    assert qlib.last_error().startswith("qqq_upper_factor: bad argument")

