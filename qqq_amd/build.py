"""Builds the gfx950 HIP libraries with hipcc, in-tree:

    qqq_amd/libqqq_amd.so      the operator (include/*.h but qqq_amd_dev.h) <- csrc/qqq_w4a8.hip: ONE translation unit -- the C-ABI entry points -- that includes
                               the kernels with their launch tables (csrc/qqq_*.hip.h) and the dispatch planner (csrc/qqq_plan.h + the generated
                               csrc/qqq_rates.h: pure host C++, compiles alone with the host compiler)
    qqq_amd/libqqq_amd_dev.so  test / tuning companion (include/qqq_amd_dev.h) <- csrc/qqq_dev.hip
    qqq_amd/_torch_ext*.so     compiled torch binding (pybind + TORCH_LIBRARY) of the operator library <- csrc/qqq_torch.cpp
    qqq_amd/libqqq_amd_quant.so  the GPTQ quantiser (quant/include/*.h, quant/include_ext/*.h and quant/include_ops/*.h), an offline tool beside the operator <- quant/csrc/qqq_quant.hip

Each library has ONE flat directory of headers and one lister: operator_headers() for include/, quant_headers() for quant/include/.  A library
is rebuilt for, and bound from, what its lister returns, so a new feature adds include/qqq_amd_<feature>.h, includes it from the translation
unit, and nothing here.  The quantiser has a second flat directory, quant/include_ext/ (quant_ext_headers()): the contents of quant/include/
are pinned by name, so the header of the next quantiser op went there -- and was pinned by name in turn.  The chain ends with a third,
quant/include_ops/ (quant_op_headers()): EVERY later quantiser op drops its header there, and no test pins that directory's listing (tests
assert membership and that no name is declared twice).  The library is rebuilt for, and bound from, all three.

The operator has a second flat directory as well, include_ops/ (operator_op_headers()): the number of headers in include/ is pinned, so
the header of the Qwen3 q / k norm went there, and every later operator op drops its header there too.  libqqq_amd.so is rebuilt for, and
bound from, both.

The .so files are git-ignored but travel to the GPU box with the repo snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "csrc", "qqq_w4a8.hip")  # the one translation unit of the operator; it includes csrc/*.hip.h, csrc/qqq_plan.h and every header operator_headers() and operator_op_headers() list
DEV_SRC = os.path.join(_HERE, "csrc", "qqq_dev.hip")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
LIB = os.environ.get("QQQ_AMD_LIB") or os.path.join(_HERE, "libqqq_amd.so")  # override: tuning builds only
DEV_LIB = os.path.join(_HERE, "libqqq_amd_dev.so")
ARCH = "gfx950"


def hipcc_path() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: cannot build the gfx950 kernels")


def header(name: str) -> str:
    return os.path.join(INCLUDE, name)


def headers() -> list:
    """every header of the C ABI: one new file under include/ is all a new feature adds here"""
    return sorted(header(f) for f in os.listdir(INCLUDE) if f.endswith(".h"))


def operator_headers() -> list:
    """the operator library's (libqqq_amd.so): all but the dev companion's"""
    return [h for h in headers() if h != header("qqq_amd_dev.h")]


OPS_INCLUDE = os.path.join(os.path.dirname(_HERE), "include_ops")  # flat, and open: the operator's headers from the Qwen3 q / k norm on


def operator_op_headers() -> list:
    """the operator library's headers outside include/, whose listing is pinned by count: one new file under include_ops/ is all a later
    operator op adds here"""
    return sorted(os.path.join(OPS_INCLUDE, f) for f in os.listdir(OPS_INCLUDE) if f.endswith(".h"))


def _stale(lib: str, extra) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    csrc = os.path.dirname(SRC)
    deps = list(extra) + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    return any(os.path.getmtime(p) > t for p in deps)


def needs_build() -> bool:
    return _stale(LIB, operator_headers() + operator_op_headers())


def _compile(src: str, out: str, verbose: bool, flags=()) -> str:
    cmd = [
        hipcc_path(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread",
        "-Wall", "-Wno-unused-function", "-o", out + ".tmp", src,
    ] + list(flags) + os.environ.get("QQQ_AMD_CXXFLAGS", "").split()
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(out + ".tmp", out)
    return out


def build(force: bool = False, verbose: bool = False) -> str:
    if force or needs_build():
        _compile(SRC, LIB, verbose)
    build_quant(force, verbose)
    return LIB


QUANT_DIR = os.path.join(_HERE, "quant")
QUANT_SRC = os.path.join(QUANT_DIR, "csrc", "qqq_quant.hip")  # the one translation unit of the quantiser; it includes quant/csrc/*.hip.h and every header quant_headers(), quant_ext_headers() and quant_op_headers() list
QUANT_INCLUDE = os.path.join(QUANT_DIR, "include")  # outside include/: headers() does not see it
QUANT_HEADER = os.path.join(QUANT_INCLUDE, "qqq_amd_quant.h")  # the ABI version is read from it
QUANT_LIB = os.path.join(_HERE, "libqqq_amd_quant.so")
# the quantiser's entry points promise bits: no fused multiply-add the source does not spell, a correctly rounded divide, subnormals kept
QUANT_FLAGS = ("-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-fno-gpu-flush-denormals-to-zero")


def quant_headers() -> list:
    """the quantiser library's (libqqq_amd_quant.so): one new file under quant/include/ is all a new quantiser op adds here"""
    return sorted(os.path.join(QUANT_INCLUDE, f) for f in os.listdir(QUANT_INCLUDE) if f.endswith(".h"))


QUANT_EXT_INCLUDE = os.path.join(QUANT_DIR, "include_ext")  # flat, like the two others


def quant_ext_headers() -> list:
    """the quantiser library's headers outside the pinned quant/include/: one new file under quant/include_ext/ is all a new quantiser op adds here"""
    return sorted(os.path.join(QUANT_EXT_INCLUDE, f) for f in os.listdir(QUANT_EXT_INCLUDE) if f.endswith(".h"))


QUANT_OPS_INCLUDE = os.path.join(QUANT_DIR, "include_ops")  # flat, and open: the headers of every quantiser op from the smoothing op on


def quant_op_headers() -> list:
    """the quantiser library's headers outside the two pinned directories: one new file under quant/include_ops/ is all a new quantiser op adds here"""
    return sorted(os.path.join(QUANT_OPS_INCLUDE, f) for f in os.listdir(QUANT_OPS_INCLUDE) if f.endswith(".h"))


def build_quant(force: bool = False, verbose: bool = False) -> str:
    """the GPTQ quantiser's library (qqq_amd/quant): an offline tool with a library of its own, libqqq_amd.so stays as it is"""
    csrc = os.path.dirname(QUANT_SRC)
    deps = quant_headers() + quant_ext_headers() + quant_op_headers() + [header("qqq_amd.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    if not force and os.path.exists(QUANT_LIB) and os.path.getmtime(QUANT_LIB) >= max(map(os.path.getmtime, deps)):
        return QUANT_LIB
    return _compile(QUANT_SRC, QUANT_LIB, verbose, QUANT_FLAGS)


def build_dev(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(DEV_LIB, [header("qqq_amd.h"), header("qqq_amd_dev.h")]):
        return DEV_LIB
    return _compile(DEV_SRC, DEV_LIB, verbose)


TORCH_SRC = os.path.join(_HERE, "csrc", "qqq_torch.cpp")


def torch_ext_path() -> str:
    import sysconfig

    return os.path.join(_HERE, "_torch_ext" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))


def build_torch_ext(force: bool = False, verbose: bool = False) -> str:
    """g++ against torch's own headers (a ROCm torch ships c10/hip/*.h): no kernel code, no hipify -- the module only forwards
    data_ptr()s and the current HIP stream to libqqq_amd.so, which it finds next to itself ($ORIGIN)."""
    import sysconfig

    import torch
    from torch.utils import cpp_extension as ce

    out = torch_ext_path()
    default_lib = os.path.join(_HERE, "libqqq_amd.so")
    if not os.path.exists(default_lib):
        raise RuntimeError("build the operator library first (qqq_amd.build.build())")
    if not force and os.path.exists(out) and os.path.getmtime(out) >= max(map(os.path.getmtime, (TORCH_SRC, header("qqq_amd.h"), header("qqq_amd_score.h")))):
        return out
    tdir = os.path.dirname(torch.__file__)
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}", "-DTORCH_EXTENSION_NAME=_torch_ext",
           "-DTORCH_API_INCLUDE_EXTENSION_H", "-Wno-deprecated-declarations"]
    cmd += [f"-I{p}" for p in ce.include_paths()] + [f"-I{sysconfig.get_paths()['include']}", "-I/opt/rocm/include"]
    cmd += [TORCH_SRC, "-o", out + ".tmp", f"-L{tdir}/lib", "-lc10", "-lc10_hip", "-ltorch_cpu", "-ltorch", "-ltorch_python",
            f"-L{_HERE}", "-lqqq_amd", "-Wl,-rpath,$ORIGIN", f"-Wl,-rpath,{tdir}/lib"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(out + ".tmp", out)
    return out


if __name__ == "__main__":
    print(build(force=True, verbose=True))
    print(build_dev(force=True, verbose=True))
    print(build_torch_ext(force=True, verbose=True))
