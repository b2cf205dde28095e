"""Builds the gfx950 HIP libraries with hipcc, in-tree:

    qqq_amd/libqqq_amd.so      the operator (include/qqq_amd.h)      <- csrc/qqq_w4a8.hip: ONE translation unit -- the C-ABI entry points -- that includes
                               the kernels with their launch tables (csrc/qqq_*.hip.h) and the dispatch planner (csrc/qqq_plan.h + the generated
                               csrc/qqq_rates.h: pure host C++, compiles alone with the host compiler)
    qqq_amd/libqqq_amd_dev.so  test / tuning companion (include/qqq_amd_dev.h) <- csrc/qqq_dev.hip
    qqq_amd/_torch_ext*.so     compiled torch binding (pybind + TORCH_LIBRARY) of the operator library <- csrc/qqq_torch.cpp
    qqq_amd/libqqq_amd_quant.so  the GPTQ quantiser (quant/include/qqq_amd_quant.h), an offline tool beside the operator <- quant/csrc/qqq_quant.hip
                                 (and its rotation op, quant/include/qqq_amd_rotate.h)

The .so files are git-ignored but travel to the GPU box with the repo snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "csrc", "qqq_w4a8.hip")  # the one translation unit of the operator; it includes csrc/*.hip.h and csrc/qqq_plan.h
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


def serving_headers() -> list:
    """the serving headers of the operator library (include/serving/*.h): entry points beside the operator's own, bound behind them"""
    sub = os.path.join(INCLUDE, "serving")
    return sorted(os.path.join(sub, f) for f in os.listdir(sub) if f.endswith(".h"))


def extension_headers() -> list:
    """the headers in the subdirectories of include/serving/ (include/serving/<feature>/*.h): one new file is all the next feature adds"""
    sub = os.path.join(INCLUDE, "serving")
    dirs = sorted(d for d in os.listdir(sub) if os.path.isdir(os.path.join(sub, d)))
    return [os.path.join(sub, d, f) for d in dirs for f in sorted(os.listdir(os.path.join(sub, d))) if f.endswith(".h")]


def feature_headers() -> list:
    """every header in a subdirectory of include/ other than serving/ (include/<feature>/*.h): the next feature adds a file and no lister"""
    dirs = sorted(d for d in os.listdir(INCLUDE) if d != "serving" and os.path.isdir(os.path.join(INCLUDE, d)))
    return sorted(os.path.join(INCLUDE, d, f) for d in dirs for f in os.listdir(os.path.join(INCLUDE, d)) if f.endswith(".h"))


def nested_headers() -> list:
    """every header two levels below include/, in a group other than serving/ (include/<group>/<feature>/*.h): bound behind bound_headers()"""
    out = []
    for group in sorted(d for d in os.listdir(INCLUDE) if d != "serving" and os.path.isdir(os.path.join(INCLUDE, d))):
        for feature in sorted(d for d in os.listdir(os.path.join(INCLUDE, group)) if os.path.isdir(os.path.join(INCLUDE, group, d))):
            sub = os.path.join(INCLUDE, group, feature)
            out += [os.path.join(sub, f) for f in sorted(os.listdir(sub)) if f.endswith(".h")]
    return out


def deep_headers() -> list:
    """every header three or more levels below include/, wherever it sits (include/<group>/<area>/<feature>/.../*.h): bound behind
    nested_headers().  It walks the whole tree below that depth, so a later feature adds a file and no lister."""
    out = []
    for top, _, files in os.walk(INCLUDE):
        if os.path.relpath(top, INCLUDE).count(os.sep) >= 2:
            out += [os.path.join(top, f) for f in files if f.endswith(".h")]
    return sorted(out)


def bound_headers() -> list:
    """what libqqq_amd.so is bound from and rebuilt for, in binding order"""
    return operator_headers() + serving_headers() + extension_headers() + feature_headers()


def _stale(lib: str, extra) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    csrc = os.path.dirname(SRC)
    deps = list(extra) + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    return any(os.path.getmtime(p) > t for p in deps)


def needs_build() -> bool:
    return _stale(LIB, bound_headers() + nested_headers() + deep_headers())


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
QUANT_SRC = os.path.join(QUANT_DIR, "csrc", "qqq_quant.hip")  # the one translation unit of the quantiser; it includes quant/csrc/qqq_gptq.hip.h, qqq_gptq_order.hip.h and qqq_hadamard.hip.h
QUANT_HEADER = os.path.join(QUANT_DIR, "include", "qqq_amd_quant.h")  # outside include/: the listers above do not see it
ROTATE_HEADER = os.path.join(QUANT_DIR, "include", "qqq_amd_rotate.h")  # the rotation op of the same library: a header of its own
ORDER_HEADER = os.path.join(QUANT_DIR, "include", "qqq_amd_gptq_order.h")  # act-order / static groups: the per-column sweep and the batched group scales
QUANT_LIB = os.path.join(_HERE, "libqqq_amd_quant.so")
# the quantiser's entry points promise bits: no fused multiply-add the source does not spell, a correctly rounded divide, subnormals kept
QUANT_FLAGS = ("-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-fno-gpu-flush-denormals-to-zero")


def build_quant(force: bool = False, verbose: bool = False) -> str:
    """the GPTQ quantiser's library (qqq_amd/quant): an offline tool with a library of its own, libqqq_amd.so stays as it is"""
    csrc = os.path.dirname(QUANT_SRC)
    deps = [QUANT_HEADER, ROTATE_HEADER, ORDER_HEADER, header("qqq_amd.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
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
