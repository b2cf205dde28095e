"""The C ABI as ctypes, read from include/qqq_amd*.h: the prototype in the header is the one statement of a signature (the compiler holds the
definition in csrc/ against it; bind() derives argtypes / restype from it).  Standard library only; no general C parser -- a declaration
the headers do not use yet raises when the library is loaded, and gets a row in the table below."""
from __future__ import annotations

import ctypes
import re

from . import build as _build


def source(path: str) -> str:
    """a header's text without its comments"""
    with open(path) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)


def define(path: str, name: str) -> int:
    return int(re.search(rf"^\s*#\s*define\s+{name}\s+(\d+)\s*$", source(path), re.M).group(1))


def int_fields(path: str, tag: str) -> list:
    """_fields_ of `struct tag { int a; int b; ... }`"""
    decls = [d.split() for d in re.search(rf"struct\s+{tag}\s*\{{(.*?)\}}", source(path), re.S).group(1).split(";") if d.strip()]
    if not decls or any(len(d) != 2 or d[0] != "int" for d in decls):
        raise RuntimeError(f"{path}: struct {tag}: every member must be `int name;`, found {decls}")
    return [(d[1], ctypes.c_int) for d in decls]


class QQQTune(ctypes.Structure):
    _fields_ = int_fields(_build.header("qqq_amd.h"), "qqq_tune")


def prototypes(path: str) -> dict:
    """{name: (return type, [parameter declarations])} of every function the header declares"""
    text = re.sub(r"^\s*#.*$", "", source(path), flags=re.M)
    text = re.sub(r"typedef\s+struct\b[^{;]*\{[^}]*\}[^;]*;", "", text)  # typedef struct {...} name;
    text = re.sub(r"typedef[^;{]*\(\s*\*[^;]*;", "", text)              # typedef ret (*name)(...);
    text = re.sub(r'extern\s+"C"\s*\{|\}', "", text)
    out = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = re.fullmatch(r"(.+?)\b(\w+) ?\(([^()]*)\)", stmt)
        if not m:
            raise RuntimeError(f"{path}: not a function prototype: `{stmt}`")
        ret, name, params = (g.strip() for g in m.groups())
        out[name] = (ret, [] if params in ("", "void") else [p.strip() for p in params.split(",")])
    return out


_PARAM = {
    "const void*": ctypes.c_void_p, "void*": ctypes.c_void_p,
    "int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
    "const qqq_tune_t*": ctypes.POINTER(QQQTune), "qqq_tune_t*": ctypes.POINTER(QQQTune),
    "int32_t*": ctypes.c_void_p,  # acc_out: a device pointer
    "double*": ctypes.POINTER(ctypes.c_double), "int*": ctypes.POINTER(ctypes.c_int), "float*": ctypes.POINTER(ctypes.c_float),
    "const void* const*": ctypes.POINTER(ctypes.c_void_p), "const uint32_t*": ctypes.POINTER(ctypes.c_uint32),
    "qqq_gemm_ex_fn": ctypes.c_void_p, "qqq_gemm_ex2_fn": ctypes.c_void_p,
}
_RETURN = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}


def _spelling(ctype: str) -> str:
    return re.sub(r"\s*\*\s*", "* ", ctype).strip()


def ctype_of(declaration: str):
    """the ctypes type of one parameter declaration (`const void* x`); a type that has no row in the table raises"""
    m = re.fullmatch(r"(.+?)\s*\b(\w+)", declaration.strip())
    if not m or _spelling(m.group(1)) not in _PARAM:
        raise RuntimeError(f"no ctypes type for the parameter `{declaration}`")
    return _PARAM[_spelling(m.group(1))]


def bind(library, path: str) -> None:
    """argtypes and restype of every function the header declares, set on the loaded library"""
    for name, (ret, params) in prototypes(path).items():
        fn = getattr(library, name)
        try:
            if _spelling(ret) not in _RETURN:
                raise RuntimeError(f"no ctypes type for the return type `{ret}`")
            fn.restype, fn.argtypes = _RETURN[_spelling(ret)], [ctype_of(p) for p in params]
        except RuntimeError as e:
            raise RuntimeError(f"{path}: {name}: {e}") from None
