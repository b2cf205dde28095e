"""The C-ABI library loads without a GPU and exports every symbol include/qqq_amd.h declares; the
reference's shape validation (return codes 0/1/2) is reproduced before any HIP call."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def _declared(header):
    from qqq_amd import _abi

    return set(_abi.prototypes(os.path.join(ROOT, "include", header)))


# ---- the parser the bindings are made with (qqq_amd/_abi.py), on header texts written here

vp, ci, cf, cz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t

TOY = """\
/* a header in the style of include/qqq_amd*.h: int toy_commented_out(int x); */
#ifndef TOY_H_
#define TOY_H_
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define TOY_VERSION 7  /* not 8 */
typedef struct toy_tune {
  int a;  /* int hidden; */
  int b;  // int hidden2;
} toy_tune_t;
typedef int (*toy_fn)(const void* A, int n);   /* no export */
int toy_multi(const void* A, void* argmax /* may be NULL */,
              int n,   // rows
              float x,
              size_t bytes);
size_t toy_bytes(int rows);
int  toy_version( void );
const char *toy_error(void);
#ifdef __cplusplus
}
#endif
#endif
"""


@pytest.fixture
def toy(tmp_path):
    p = tmp_path / "toy.h"
    p.write_text(TOY)
    return str(p)


def test_parser_reads_prototypes_and_nothing_else(toy):
    from qqq_amd import _abi

    assert _abi.prototypes(toy) == {
        "toy_multi": ("int", ["const void* A", "void* argmax", "int n", "float x", "size_t bytes"]),  # spans lines, comments inside the list
        "toy_bytes": ("size_t", ["int rows"]),
        "toy_version": ("int", []),          # (void)
        "toy_error": ("const char *", []),
    }  # neither typedef, nothing from a comment
    assert _abi.define(toy, "TOY_VERSION") == 7
    assert _abi.int_fields(toy, "toy_tune") == [("a", ci), ("b", ci)]


def test_parser_refuses_what_it_does_not_know(tmp_path):
    from qqq_amd import _abi

    p = tmp_path / "odd.h"
    p.write_text("static inline int toy_inline(int x) { return x; }\n")
    with pytest.raises(RuntimeError, match="not a function prototype"):
        _abi.prototypes(str(p))
    p.write_text("typedef struct toy { int a; float b; } toy_t;\n")
    with pytest.raises(RuntimeError, match="struct toy"):
        _abi.int_fields(str(p), "toy")


@pytest.mark.parametrize("decl, ctype", [
    ("const void* x", vp), ("void* x", vp), ("int x", ci), ("float x", cf), ("size_t x", cz),
    ("const qqq_tune_t* x", "tune"), ("qqq_tune_t* x", "tune"), ("int32_t* x", vp),
    ("double* x", ctypes.POINTER(ctypes.c_double)), ("int* x", ctypes.POINTER(ci)), ("float* x", ctypes.POINTER(cf)),
    ("const void* const* x", ctypes.POINTER(vp)), ("const uint32_t* x", ctypes.POINTER(ctypes.c_uint32)),
    ("qqq_gemm_ex_fn x", vp), ("qqq_gemm_ex2_fn x", vp),
    ("const void *x", vp), ("const void * const * x", ctypes.POINTER(vp)),  # the spelling of the star does not matter
])
def test_type_table(decl, ctype):
    from qqq_amd import _abi, _lib

    assert _abi.ctype_of(decl) is (ctypes.POINTER(_lib.QQQTune) if ctype == "tune" else ctype)


@pytest.mark.parametrize("decl", ["long long n", "unsigned n", "int", "const int* x", "void** x", "char x", "int x[4]"])
def test_unknown_parameter_type_raises_with_header_function_and_parameter(tmp_path, decl):
    from qqq_amd import _abi

    with pytest.raises(RuntimeError, match="no ctypes type"):
        _abi.ctype_of(decl)
    p = tmp_path / "future.h"
    p.write_text(f"int toy_future(const void* A, {decl});\n")

    class Lib:
        class toy_future:
            argtypes = restype = None

    with pytest.raises(RuntimeError) as ei:
        _abi.bind(Lib, str(p))
    assert "future.h" in str(ei.value) and "toy_future" in str(ei.value) and f"`{decl}`" in str(ei.value)
    assert Lib.toy_future.argtypes is None and Lib.toy_future.restype is None  # nothing half-bound
    p.write_text("long toy_future(int n);\n")
    with pytest.raises(RuntimeError, match="future.h: toy_future: .*return type `long`"):
        _abi.bind(Lib, str(p))


# ---- the two libraries as bound from the headers

def _headers():
    return sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))


OPERATOR_HEADERS = [h for h in _headers() if h != "qqq_amd_dev.h"]


@pytest.fixture(scope="module")
def D():
    from qqq_amd import _dev, build

    build.build()
    build.build_dev()
    return _dev.lib()


def test_headers_are_found_by_listing_include():
    from qqq_amd import build

    inc = os.path.join(ROOT, "include")
    assert len(_headers()) == 20 and len(OPERATOR_HEADERS) == 19 and "qqq_amd.h" in OPERATOR_HEADERS
    assert build.headers() == [os.path.join(inc, h) for h in _headers()]
    assert build.operator_headers() == [os.path.join(inc, h) for h in OPERATOR_HEADERS]


def test_the_include_directories_are_flat():
    """headers() and quant_headers() list one directory each: a header in a subdirectory would go unbound and unwatched"""
    from qqq_amd import build

    dirs = (os.path.join(ROOT, "include"), os.path.join(ROOT, "qqq_amd", "quant", "include"))
    assert dirs == (build.INCLUDE, build.QUANT_INCLUDE)
    for inc in dirs:
        assert [d for d in os.listdir(inc) if os.path.isdir(os.path.join(inc, d))] == [], inc


@pytest.mark.parametrize("lister", ["operator_headers", "quant_headers"])
def test_no_function_is_declared_in_two_headers_of_one_library(lister):
    """every header of a library is bound onto the same handle, in listing order: a name declared twice would be bound twice"""
    from qqq_amd import _abi, build

    seen = {}
    for h in getattr(build, lister)():
        for name in _abi.prototypes(h):
            assert name not in seen, (name, seen[name], h)
            seen[name] = h
    assert seen


@pytest.mark.parametrize("header", _headers())
def test_every_declared_function_is_bound_as_declared(L, D, header):
    from qqq_amd import _abi

    lib = D if header == "qqq_amd_dev.h" else L
    protos = _abi.prototypes(os.path.join(ROOT, "include", header))
    assert protos and all(n.startswith("qqq_") for n in protos)
    for name, (ret, params) in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        assert fn.restype is {"int": ci, "size_t": cz, "const char*": ctypes.c_char_p}[ret], name


def test_signatures_pinned_by_hand(L, D):
    """every row of the type table on the real headers, written out as the bindings used to be"""
    from qqq_amd import _lib

    tune, pf = ctypes.POINTER(_lib.QQQTune), ctypes.POINTER(cf)
    assert L.qqq_decode_attn.argtypes == [vp, vp, vp, vp, cf, vp, vp, vp, vp, cz, ci, ci, ci, ci, ci, ci, ci, vp]
    assert L.qqq_w4a8_gemm_ex2.argtypes == [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, ci, vp, ci, ci, ci, ci, tune, vp, vp, vp]
    assert L.qqq_decode_attn_shared_plan.argtypes == [ci, ci, ci, ci, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    assert L.qqq_w4a8_plan.argtypes == [ci, ci, ci, ci, ci, ci, ci, tune, tune]
    assert L.qqq_w4a8_model_us.argtypes == [ci, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_double)]
    assert D.qqq_dev_probe_fill.argtypes == [vp, cz, cz, ci, ci, ci, vp, ci, vp, pf]
    assert D.qqq_dev_bench_gemm2.argtypes == [vp, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ci, vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, ci, vp, ci,
                                              tune, ci, pf]
    assert D.qqq_dev_probe_placement.argtypes == [ctypes.POINTER(ctypes.c_uint32), ci, ci, ci, vp, ci, vp]
    for fn in (L.qqq_decode_attn, L.qqq_w4a8_gemm_ex2, L.qqq_decode_attn_shared_plan, D.qqq_dev_probe_fill, D.qqq_dev_bench_gemm2):
        assert fn.restype is ci
    assert L.qqq_decode_attn_workspace_bytes.restype is cz and L.qqq_decode_attn_workspace_bytes.argtypes == [ci] * 5
    for fn, ret in ((L.qqq_amd_abi_version, ci), (L.qqq_amd_last_error, ctypes.c_char_p), (D.qqq_dev_last_error, ctypes.c_char_p)):
        assert fn.argtypes == [] and fn.restype is ret


def test_tune_struct_and_abi_version_are_the_header_s():
    from qqq_amd import _lib

    assert _lib.QQQTune._fields_ == [(f, ci) for f in ("kernel", "ksplit", "waves", "fused", "bm", "glds", "pf", "stages", "mt", "pw", "nslots",
                                                       "split_m", "skew", "w8")]
    assert _lib.ABI_VERSION == 4


def test_the_compiler_checks_every_definition_against_its_prototype():
    """the two translation units include every header they define, so a definition that disagrees with its prototype does not compile
    (extern "C": a second declaration with other parameters is an error)"""
    from qqq_amd import build

    unit = open(build.SRC).read()
    # qqq_amd.h comes in with the unit's first include, the kernels' common header; the feature headers are included by the unit itself
    assert '#include "qqq_common.hip.h"' in unit
    unit += open(os.path.join(os.path.dirname(build.SRC), "qqq_common.hip.h")).read()
    for h in OPERATOR_HEADERS:
        assert f'#include "../../include/{h}"' in unit, h
    assert '#include "../../include/qqq_amd_dev.h"' in open(build.DEV_SRC).read()


@pytest.mark.parametrize("header", OPERATOR_HEADERS)
def test_a_newer_header_rebuilds_the_operator_library(monkeypatch, L, header):
    from qqq_amd import build

    newer = os.path.join(ROOT, "include", header)
    monkeypatch.setattr(os.path, "getmtime", lambda p: 2.0 if p == build.LIB else 1.0)
    assert not build.needs_build()
    monkeypatch.setattr(os.path, "getmtime", lambda p: 2.0 if p == build.LIB else 3.0 if p == newer else 1.0)
    assert build.needs_build()


def test_exports_every_declared_symbol(L):
    names = _declared("qqq_amd.h")
    assert {"qqq_w4a8_gemm", "qqq_w4a8_gemm_ex", "qqq_w4a8_gemm_ex2", "qqq_expand_int8", "qqq_w4a8_plan", "qqq_w4a8_model_us", "qqq_dynamic_quant",
            "qqq_quantlinear_forward", "qqq_quantlinear_forward2", "qqq_pack_int4", "qqq_unpack_int4", "qqq_amd_abi_version",
            "qqq_amd_last_error"} == names
    for n in names:
        assert hasattr(L, n), n
    assert L.qqq_amd_abi_version() == 4
    # the operator library is the operator only: measurement loops and hardware probes live in the dev library
    for n in ("qqq_bench_gemm", "qqq_probe_mfma", "qqq_probe_glds", "qqq_probe_fill", "qqq_add_bias", "qqq_dev_bench_gemm"):
        assert not hasattr(L, n), n


def test_dev_library_exports_every_declared_symbol():
    from qqq_amd import _dev, build

    build.build_dev()
    D = _dev.lib()
    names = _declared("qqq_amd_dev.h")
    assert {"qqq_dev_bench_gemm", "qqq_dev_bench_gemm2", "qqq_dev_probe_mfma", "qqq_dev_probe_glds", "qqq_dev_probe_dequant",
            "qqq_dev_probe_fill", "qqq_dev_probe_mfma_rate", "qqq_dev_probe_placement", "qqq_dev_last_error"} == names
    for n in names:
        assert hasattr(D, n), n


def _call(L, m, n, k, groupsize=-1, thread_k=-1, thread_n=-1):
    z = None  # shape validation happens before any pointer is touched
    return L.qqq_w4a8_gemm(z, z, z, z, z, z, z, m, n, k, z, groupsize, 0, z, thread_k, thread_n, -1, 16)


def test_reference_shape_validation_codes(L):
    # reference: is_valid_config / determine_thread_config / CALL_IF (csrc/qqq_gemm.cu:867-945, :990)
    assert _call(L, 16, 100, 256) == 1            # n not a multiple of 64
    assert _call(L, 16, 256, 96) == 1             # k not a multiple of 64
    assert _call(L, 16, 64, 64) == 1              # n=64 needs thread_k=128 -> k % 128
    assert _call(L, 0, 256, 256) == 0             # empty problem: success, nothing launched (:1002)
    assert _call(L, 16, 256, 0) == 0 or _call(L, 16, 256, 0) == 1
    assert _call(L, 16, 256, 256, thread_k=32, thread_n=128) == 1   # thread_k must be 64 or 128
    assert _call(L, 16, 256, 256, thread_k=64, thread_n=128) == 2   # valid tiling, no such kernel at 256 threads
    assert _call(L, 16, 256, 256, groupsize=64) == 2                # only group 128 kernels exist
    assert _call(L, 0, 256, 256, groupsize=64) == 0
    # valid shape, null pointers: our own argument check, still no launch
    assert _call(L, 16, 256, 256) == 17


def test_misaligned_pointers_are_rejected_before_any_launch(L):
    """include/qqq_amd.h documents QQQ_ERR_ARG for misaligned pointers: the kernels use 16-byte vector / LDS-DMA
    accesses on A, B, C, D, s3, bias and 8-byte loads on s2.  Checked on the host, so no GPU is needed."""
    import numpy as np

    buf = np.zeros(1 << 16, np.uint8)
    base = (buf.ctypes.data + 63) & ~63
    ok = [base + 4096 * i for i in range(8)]  # A B C D s1 s2 s3 ws

    def call(ptrs, groupsize=-1, bias=None):
        A, B, C, D, s1, s2, s3, ws = ptrs
        return L.qqq_w4a8_gemm_ex(A, B, C, D, s1, s2, s3, 16, 256, 256, ws, groupsize, 0, None, -1, -1, -1, 16, None, None, bias)

    for idx, off in ((0, 8), (1, 4), (2, 8), (3, 2), (5, 4), (4, 2), (7, 1)):
        bad = list(ok)
        bad[idx] += off
        assert call(bad) == 17, idx
        assert b"misaligned" in L.qqq_amd_last_error()
    bad = list(ok)
    bad[6] += 2
    assert call(bad, groupsize=128) == 17  # s3 only matters in per-group mode
    assert call(ok, bias=base + 2) == 17


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from qqq_amd import _lib, build

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(build, "LIB", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def _check_plan(m, n, k, grouped, max_par):
    """the invariants every automatic plan must keep: the reference's buffers (C = max_par*64 rows x n int32, workspace =
    n/128*max_par ints; qlinear_marlin.py:117-133) bound every split, and no plan needs scratch it was not given"""
    from qqq_amd import _lib

    gs = 128 if grouped else -1
    p = _lib.plan(m, n, k, gs, max_par)
    assert p["kernel"] in (1, 2, 3, 4, 5) and p["ksplit"] >= 1
    # the M split: only where the whole call is the wide kernel's, whole tiles first, a remainder of at most 2048 tokens second -- and each of the two
    # launches is a plan of its own that keeps every invariant below (checked by recursion: the parts are never split again)
    sm = p["split_m"]
    assert sm >= 0 and (sm == 0 or (p["kernel"] == 5 and 0 < sm < m and sm % (16 * p["mt"]) == 0 and m - sm <= 2048)), p
    if sm:
        for part in (sm, m - sm):
            q = _lib.plan(part, n, k, gs, max_par, tune=dict(split_m=-1))
            assert q["split_m"] == 0
        _check_plan_part(sm, n, k, grouped, max_par)
        _check_plan_part(m - sm, n, k, grouped, max_par)
    return _check_plan_part(m, n, k, grouped, max_par)


def _check_plan_part(m, n, k, grouped, max_par):
    from qqq_amd import _lib

    gs = 128 if grouped else -1
    p = _lib.plan(m, n, k, gs, max_par, tune=dict(split_m=-1))
    cap_rows, cap_tk = max_par * 64, (n // 128) * max_par
    if p["kernel"] == 5:  # wide: 256 x 256 / 256 x 128 / 128 x 256 tiles; 32-bit offsets into the packed weights; one slot of C per depositing slice
        assert m > 256 and n % 64 == 0 and k % 128 == 0 and n * k // 2 < 2**32
        assert p["pf"] in (4, 8) and p["stages"] == 1 and p["pw"] in (4, 8, 16, 32) and (p["mt"], p["bm"]) in ((16, 256), (16, 128), (8, 256))
        rows = 16 * p["mt"]
        tiles = -(-m // rows) * -(-n // p["bm"])
        if p["ksplit"] > 1:
            assert tiles * rows * p["bm"] * (p["ksplit"] - 1) <= cap_rows * n and 2 * tiles <= cap_tk and p["ksplit"] <= (k // 128) // 4
        assert _lib.plan(m, n, k, gs, max_par, have_scratch=False)["ksplit"] == 1
        return p
    if p["kernel"] == 4:  # panel: one slot of C per depositing slice, two ticket words per tile
        rows, bn = 16 * p["mt"], p["bm"]
        mblocks, strips = -(-m // rows), -(-n // bn)
        assert n % 64 == 0 and k % 64 == 0 and bn in (128, 256) and p["mt"] in (1, 2, 4, 8)
        if p["ksplit"] > 1:
            assert mblocks * strips * rows * bn * (p["ksplit"] - 1) <= cap_rows * n and 2 * mblocks * strips <= cap_tk
            assert p["ksplit"] <= ((k // 64 + 1) // 2)
        assert _lib.plan(m, n, k, gs, max_par, have_scratch=False)["ksplit"] == 1
        return p
    if p["kernel"] == 3:
        assert m <= 32 and n % 64 == 0 and k % 64 == 0 and p["ksplit"] == 1
        return p
    if p["kernel"] == 1:
        assert m <= 256 or k % 128 or n % 64  # the stream family is only chosen for a few m-blocks
        if p["ksplit"] > 1:
            assert p["ksplit"] * m <= cap_rows and p["fused"] == 2
            if p["mt"] >= 2:  # 8-wave bodies, one workgroup per CU: the split never asks for a second round
                assert -(-n // 128) * -(-m // (16 * p["mt"])) * p["ksplit"] <= 256
        return p
    rows = 256 if p["bm"] >= 256 else 128 if p["bm"] >= 128 else 64
    tiles = -(-m // rows) * -(-n // 256)
    assert p["ksplit"] <= k // 128
    if p["ksplit"] > 1 and p["nslots"] > 0:  # in-launch: slots + tickets must fit
        assert p["nslots"] * tiles * rows * 256 <= cap_rows * n
        assert tiles * (1 + p["nslots"]) <= cap_tk and p["nslots"] <= p["ksplit"] - 1
    elif p["ksplit"] > 1:  # slabs
        assert p["ksplit"] * m <= cap_rows
    # without scratch there is never a split
    assert _lib.plan(m, n, k, gs, max_par, have_scratch=False)["ksplit"] == 1
    return p


def test_dispatch_plan_respects_scratch_contract(L):
    """qqq_w4a8_plan is pure host logic: for every shape the plan must stay inside what the reference's buffers guarantee."""
    from qqq_amd import _lib

    for grouped in (False, True):
        for n, k in ((8192, 21760), (4096, 4096), (11008, 4096), (4096, 11008), (256, 128), (320, 1536)):
            for max_par in (1, 4, 16):
                for m in (1, 7, 16, 64, 128, 129, 200, 256, 300, 512, 640, 1000, 1024, 1025, 2048, 4096, 32768):
                    _check_plan(m, n, k, grouped, max_par)
    # forced variants are honoured, and an impossible in-launch request falls back to slabs or no split
    p = _lib.plan(1024, 8192, 21760, -1, 16, tune=dict(kernel=2, bm=256, ksplit=2, fused=1))
    assert (p["bm"], p["ksplit"], p["nslots"], p["fused"]) == (256, 2, 1, 1)
    p = _lib.plan(1024, 8192, 21760, -1, 16, tune=dict(kernel=2, bm=256, ksplit=2, fused=2))
    assert p["nslots"] == 0 and p["ksplit"] == 1  # 2 slabs of 1024 rows do not fit in 1024 rows
    p = _lib.plan(2048, 8192, 21760, -1, 16, tune=dict(kernel=2, bm=256, ksplit=2, fused=1))
    assert p["ksplit"] == 1


def test_dispatch_plan_invariants_on_random_shapes(L):
    """the same invariants on shapes nobody picked by hand (hypothesis): any m, n and k in the reference's 64-multiples,
    group size 128 needs k % 128 == 0, max_par 1..16"""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=400, deadline=None, derandomize=True)
    @given(m=st.one_of(st.integers(1, 600), st.integers(1, 70000)), n64=st.integers(1, 400), k64=st.integers(1, 400),
           grouped=st.booleans(), max_par=st.integers(1, 16))
    def run(m, n64, k64, grouped, max_par):
        n, k = 64 * n64, 64 * k64
        if grouped:
            k = max(128, k // 128 * 128)
        if n == 64 and k % 128:  # reference: n = 64 needs thread_k = 128 (csrc/qqq_gemm.cu:867-897)
            k += 64
        _check_plan(m, n, k, grouped, max_par)

    run()


def test_dispatch_of_the_baseline_sweep(L):
    """The families the cost models pick at the BASELINE layer (N=8192, K=21760), as measured in profiles/r02_dispatch_check*.txt
    and profiles/r03_*: decode -> column, a few tens of tokens -> stream, 128 tokens -> panel with 4 K slices, from ~768 tokens
    -> the panel kernel with 64 columns per wave (pw = 2, no split), from ~1.5 K tokens -> the wide kernel (both modes)."""
    from qqq_amd import _lib

    N, K = 8192, 21760
    assert _lib.plan(1, N, K, -1, 16)["kernel"] == 3 and _lib.plan(8, N, K, 128, 16)["kernel"] == 3
    assert _lib.plan(16, N, K, -1, 16)["kernel"] == 1
    # 9 ... 32 tokens: column kernel vs stream kernel by two small cost models (round 4, profiles/r04_dispatch_check_m16.txt; the bound on m * K they
    # replace sent 8192 x 8192 at 24 / 32 tokens to the stream kernel, 16.0 vs 13.4 us per-channel, 18.4 vs 13.6 per-group); BASELINE decisions unchanged
    assert _lib.plan(16, N, K, 128, 16)["kernel"] == 3 and _lib.plan(24, N, K, 128, 16)["kernel"] == 1 and _lib.plan(32, N, K, -1, 16)["kernel"] == 1
    assert _lib.plan(32, 8192, 8192, -1, 16)["kernel"] == 3 and _lib.plan(24, 8192, 8192, 128, 16)["kernel"] == 3
    assert _lib.plan(32, 5120, 5120, 128, 16)["kernel"] == 3 and _lib.plan(32, 4096, 11008, -1, 16)["kernel"] == 1
    assert _lib.plan(9, 28672, 8192, -1, 16)["kernel"] == 1   # more than 512 column workgroups: never beyond 8 tokens
    # narrow layers (the k / v projections of grouped-query attention, profiles/r04_dispatch_check_merged.txt): decode on N = 1024 is the column
    # kernel's (32 workgroups, 6.3 vs 8.8 us); 256 tokens on N <= 2048 were the stream kernel's (13.7 vs 16.6 panel) until round 5 found the panel kernel's
    # 64-token m-blocks ahead of both there (profiles/r05_dispatch_check_merged.txt: 12.4 vs 13.6 us)
    assert _lib.plan(1, 1024, 4096, -1, 16)["kernel"] == 3 and _lib.plan(16, 1024, 4096, 128, 16)["kernel"] == 3
    for gs in (-1, 128):
        p = _lib.plan(256, 1024, 4096, gs, 16)
        assert (p["kernel"], p["mt"], p["bm"]) == (4, 4, 128), p
    assert _lib.plan(16, 22016, 4096, 128, 16)["kernel"] == 3 and _lib.plan(16, 22016, 4096, -1, 16)["kernel"] == 1
    # N = 512 (16 column workgroups) still decodes on the column kernel; per-group decode on long-K layers is the stream kernel's (re-quantiser-bound
    # column kernel: N = 3584, K = 18944 15.4 vs 19.4 us, profiles/r04_dispatch_check_qwen_mistral.txt); wide layers stay unsplit up to 16 tokens
    assert _lib.plan(1, 512, 3584, -1, 16)["kernel"] == 3 and _lib.plan(1, 3584, 18944, 128, 16)["kernel"] == 1 and _lib.plan(1, 3584, 18944, -1, 16)["kernel"] == 3
    p = _lib.plan(16, 18944, 3584, -1, 16)
    assert (p["kernel"], p["ksplit"]) == (1, 1), p
    # ... and never ask for a 257th workgroup, the 4-wave bodies of <= 16 tokens included (N = 7168, K = 20480: 56 strips x 4 slices, 18.9 us against 25.5
    # with 5); per-group decode on a wide layer is the column kernel's (N = 20480, K = 7168: 21.1 vs 24.9 us -- the unsplit stream slice is re-quantiser-bound)
    p = _lib.plan(16, 7168, 20480, -1, 16)
    assert (p["kernel"], p["ksplit"]) == (1, 4), p
    # 65 ... 256 tokens on layers up to ~40 MB: the stream kernel's split comes from its loop model, not from "fill 256 workgroups" -- short-K layers stay whole
    # (N = 8192, K = 3072 at 128 tokens: 15.7 us unsplit against 19.4 in two slices, profiles/r04_stream_panel_ksplit.txt), long-K ones are still split
    # (round 5: two 64-token m-blocks of the panel kernel in two slices, 13.5 us -- profiles/r05_dispatch_check_more_models.txt; the stream rule is still what a
    #  forced stream kernel does there)
    p = _lib.plan(128, 8192, 3072, -1, 16, tune=dict(kernel=1))
    assert (p["kernel"], p["ksplit"]) == (1, 1), p
    p = _lib.plan(128, 8192, 3072, -1, 16)
    assert (p["kernel"], p["mt"], p["ksplit"]) == (4, 4, 2), p
    # M split (rows are independent; profiles/r04_ragged_m.txt): a token count one past whole tiles / rounds of the wide kernel runs as two launches --
    # 4097 tokens 624 us in one launch, 464 us as 4096 + 1 -- where the models price the pair 7 % below the single launch, and only there
    # (round 5, rates refitted on the cold, order-shuffled grids: 4700 ... 5120 tokens -- 2.3 ... 2.5 rounds of 256 x 256 tiles -- split as well: 5000 tokens
    #  560 us as 4096 + 904 against 620 in one launch, per-group 725 against 810; profiles/r05_m_split_refit.txt)
    # (round 6, final rates: 5000 tokens are planned as five full rounds of 128 x 256 tiles -- 599 us by the model against 561 for 4096 + 904: 6.4 %, a whisker under the 7 % the
    #  split asks for -- and run in one launch; 4700 tokens still split)
    assert [_lib.plan(m, N, K, -1, 16)["split_m"] for m in (4096, 4097, 4224, 4352, 2049, 1025, 8200, 5000)] == [0, 4096, 4096, 4096, 2048, 1024, 8192, 0]
    assert _lib.plan(4097, N, K, 128, 16)["split_m"] == 4096 and _lib.plan(4097, N, K, -1, 16, tune=dict(split_m=-1))["split_m"] == 0
    assert _lib.plan(8200, 11008, 4096, -1, 16)["split_m"] == 0 and _lib.plan(4100, 4096, 11008, -1, 16)["split_m"] == 4096   # 43 strips: no whole rounds to keep
    assert _lib.plan(4097, N, K, -1, 16, tune=dict(kernel=5))["split_m"] == 0                                                # a forced family is never split
    # ... remainders up to 2048 tokens where the models choose them (cap 512 against 4096 measured: +5 ... +13 % there, no loss elsewhere)
    assert _lib.plan(4700, N, K, -1, 16)["split_m"] == 4096 and _lib.plan(7000, N, K, -1, 16)["split_m"] == 6144 and _lib.plan(9000, 4096, 4096, -1, 16)["split_m"] == 8192
    p = _lib.plan(128, 8192, 8192, -1, 16)   # (round 5: the panel kernel, 21.6 us against the stream kernel's 22.8 in two slices; 64-token m-blocks 20.4)
    assert (p["kernel"], p["mt"], p["ksplit"]) == (4, 8, 4), p
    assert _lib.plan(1, 20480, 7168, 128, 16)["kernel"] == 3
    p = _lib.plan(128, N, K, -1, 16)
    assert (p["kernel"], p["mt"], p["ksplit"]) == (4, 8, 4)
    # 320 - 512 tokens: 256 x 128 tiles of the wide kernel in two K slices (2 m-tiles x 64 strips x 2 = one round), both modes;
    # 640 - 1024 tokens: per-channel one unsplit round of 128-token or 128-column tiles -- 256 x 128 wherever the tile counts do not decide (cold A/B at the
    # end of round 4, profiles/r04_wide_w8_vs_w128.txt: 121.8 vs 127.2 us at 768 tokens, 134.1 vs 135.9 at 1024), 128 x 256 at 640 (160 tiles against 192);
    # per-group 256 x 256 tiles in two K slices since round 4 (the deposits stay in the XCD's L2: 150.6 / 148.7 / 167.2 us against 155.9 / 152.7 / 167.1
    # for the unsplit 256 x 128 tiles of round 3; profiles/r04_dispatch_check_mid.txt)
    for m in (320, 512):
        for gs in (-1, 128):
            p = _lib.plan(m, N, K, gs, 16)
            assert (p["kernel"], p["mt"], p["bm"], p["ksplit"]) == (5, 16, 128, 2), (m, gs, p)
    for m in (640, 768, 1024):
        p, g = _lib.plan(m, N, K, -1, 16), _lib.plan(m, N, K, 128, 16)
        # (round 5: with the 256 x 256 tiles' ring depth 8 and uneven slices two K slices of them overtook the 256 x 128 tiles at 1024 tokens: 133.8 vs 135.6 us,
        #  profiles/r05_m_split_refit.txt)
        # (round 6, rates refitted on the rebuilt loop: 768 and 1024 tokens are the unsplit 128 x 256 tiles' as well -- 105.9 vs 107.7 us (256 x 128) at 768,
        #  124.6 / 126.2 vs 128.7 / 127.9 (256 x 256 in two slices) at 1024: profiles/r06_dispatch_check_mid.txt, r06_dispatch_check_main.txt)
        assert (p["kernel"], p["mt"], p["bm"], p["ksplit"]) == (5, 8, 256, 1), (m, p)
        assert (g["kernel"], g["mt"], g["bm"], g["ksplit"]) == (5, 16, 256, 2), (m, g)
    p = _lib.plan(1024, N, K, -1, 16, tune=dict(kernel=4, bm=256, mt=8, pw=2))  # the round-2 choice stays available
    assert (p["kernel"], p["bm"], p["mt"], p["pw"], p["ksplit"]) == (4, 256, 8, 2, 1), p
    # from ~1.5 K tokens (>= 3/4 of a round of 256 x 256 tiles) the wide kernel, both modes (round 3:
    # profiles/r03_wide_*.txt -- M=4096 556 -> 478 us per-channel, 759 -> 620 us per-group)
    for m in (1280, 1536, 2048, 4096, 8192):
        for gs in (-1, 128):
            p = _lib.plan(m, N, K, gs, 16)
            assert (p["kernel"], p["mt"], p["bm"], p["ksplit"], p["pf"], p["stages"], p["pw"]) == (5, 16, 256, 1, 4, 1, 8), (m, gs, p)  # ring depth 4 since the dword weight loads of round 6 (8 loads per step: 8 steps would pass vmcnt's 63)
    # the persistent tile walk (round 4, glds == 2 in the plan): automatic on 4096 / 5120-deep layers with more than one 256 x 256
    # tile per CU, never at K = 21760 unless forced, never with a K split, and only from 8 stages of K up
    assert _lib.plan(8192, 4096, 4096, -1, 16)["glds"] == 2 and _lib.plan(8192, 11008, 4096, 128, 16)["glds"] == 2
    assert _lib.plan(4096, 4096, 4096, -1, 16)["glds"] == 1 and _lib.plan(8192, 4096, 11008, -1, 16)["glds"] == 1   # one tile per CU; K too long
    assert _lib.plan(4096, 8192, 8192, -1, 16)["glds"] == 2 and _lib.plan(8192, 8192, 8192, 128, 16)["glds"] == 2    # K = 8192: on (r04_walk_larger_k.txt)
    assert _lib.plan(8192, N, K, -1, 16)["glds"] == 1 and _lib.plan(8192, N, K, -1, 16, tune=dict(kernel=5, glds=2))["glds"] == 2
    assert _lib.plan(8192, 4096, 4096, -1, 16, tune=dict(kernel=5, glds=1))["glds"] == 1
    p = _lib.plan(2048, N, K, -1, 128, tune=dict(kernel=5, glds=2, ksplit=2))  # (max_par 128: room in C for 256 deposits)
    assert p["ksplit"] == 2 and p["glds"] == 1, p
    assert _lib.plan(8192, 4096, 896, -1, 16, tune=dict(kernel=5, glds=2))["glds"] == 1
    assert _lib.plan(1024, N, K, -1, 16, tune=dict(kernel=5, bm=128))["bm"] == 128 and _lib.plan(1024, N, K, -1, 16, tune=dict(kernel=5, mt=8, bm=128))["bm"] == 256
    # (round 6, dword weight loads: the ring is 4 steps deep whatever is asked -- 8 steps x 8 loads would pass vmcnt's 63)
    assert _lib.plan(4096, N, K, -1, 16, tune=dict(kernel=5, pf=4))["pf"] == 4 and _lib.plan(4096, N, K, 128, 16, tune=dict(kernel=5, pf=8))["pf"] == 4
    # ... and the other shapes keep per-channel 4 / per-group 8 (level in the same A/B)
    assert _lib.plan(1024, N, K, -1, 16, tune=dict(kernel=5, bm=128))["pf"] == 4 and _lib.plan(1024, N, K, 128, 16, tune=dict(kernel=5, mt=8))["pf"] == 4
    assert _lib.plan(4096, N, K, -1, 16, tune=dict(kernel=5, stages=3))["stages"] == 1  # LDS-DMA staging: one lead, a full stage
    assert _lib.plan(1024, N, K, -1, 16, tune=dict(kernel=5, mt=8))["mt"] == 8 and _lib.plan(1024, N, K, -1, 16, tune=dict(kernel=5))["mt"] == 16
    # a forced 64-column shape is honoured only where it exists (128-token m-blocks, bm = 256, prefetch depth 3 or 4)
    assert _lib.plan(300, N, K, -1, 16, tune=dict(kernel=4, bm=256, mt=8, pw=2))["pw"] == 2
    assert _lib.plan(300, N, K, -1, 16, tune=dict(kernel=4, bm=128, mt=8, pw=2))["pw"] == 1
    assert _lib.plan(300, N, K, -1, 16, tune=dict(kernel=4, bm=256, mt=4, pw=2))["pw"] == 1
    # 48 / 64 tokens (profiles/r02_dispatch_check_handoff.txt): per-channel the panel kernel takes over at 64 (29.0 vs 32.6 us),
    # the stream kernel keeps 48 (28.7 vs 30.4) and the per-group mode up to 64 (33.9 vs 36.9)
    # (round 5, the generated panel table: 48 tokens per-channel and 64 per-group go to the panel kernel too -- 27.6 vs 26.5 us and 34.4 vs 31.9 on the box of
    #  profiles/r05_dispatch_check_m64.txt, i.e. 4 / 8 % behind the stream kernel there: the two families are within their models' error of each other)
    assert _lib.plan(40, N, K, -1, 16)["kernel"] in (1, 4) and _lib.plan(64, N, K, -1, 16)["kernel"] == 4
    assert _lib.plan(48, N, K, 128, 16)["kernel"] == 1
    # the panel kernel's 32-column shapes stage activations 2 stages ahead under the 4-deep weight ring
    p = _lib.plan(128, N, K, -1, 16)
    assert (p["pf"], p["stages"]) == (4, 2)
    assert _lib.plan(128, N, K, -1, 16, tune=dict(kernel=4, stages=4))["stages"] == 4
    # the stream kernel never asks for a 257th workgroup (one 8-wave workgroup per CU): 86 strips x 3 slices -> 2 slices
    p = _lib.plan(64, 11008, 4096, -1, 16, tune=dict(kernel=1))
    assert p["kernel"] == 1 and p["ksplit"] == 2
    # 64 tokens on mid-size layers (round-4 refit over ten shapes, profiles/r04_dispatch_check_final*.txt): the panel kernel where its
    # K slices stay short (16.3 vs 17.7 us here, 14.4 vs 15.8 at 5120 x 5120), the stream kernel where K is long and n small
    # (4096 x 11008: 17.4 vs 18.3) and per-group on the very large layers (28672 x 8192: 41.6 vs 43.8)
    p = _lib.plan(64, 11008, 4096, -1, 16)
    assert (p["kernel"], p["ksplit"], p["bm"]) == (4, 2, 128), p
    assert _lib.plan(64, 5120, 5120, -1, 16)["kernel"] == 4 and _lib.plan(64, 4096, 11008, -1, 16)["kernel"] == 1
    assert _lib.plan(64, 28672, 8192, 128, 16)["kernel"] == 1 and _lib.plan(64, 8192, 28672, 128, 16)["kernel"] == 1
    p = _lib.plan(192, 4096, 4096, -1, 16, tune=dict(kernel=1))
    assert p["ksplit"] * 3 * 32 <= 256
    # short-K layers at large m: the wide kernel since its uniform schedule (profiles/r03_wide_uniform_schedule.txt: 11008 x 4096,
    # 32 K tokens 1174 vs 1429 us for the tiled kernel); the panel shapes' per-tile fixed costs weigh more there
    assert _lib.plan(8192, 4096, 4096, -1, 16)["kernel"] == 5


def test_compiled_torch_binding_imports_and_keeps_the_error_contract():
    """csrc/qqq_torch.cpp -> qqq_amd/_torch_ext*.so (the reference binds through pybind, csrc/pybind.cpp:3-5): built by
    __graft_entry__.build(), imports without a GPU, registers the qqq_amd_native ops, and raises the SAME messages as the ctypes
    path for the same bad calls (there is no CPU path in either)."""
    import torch

    from qqq_amd import build as kb, ops

    kb.build()
    kb.build_torch_ext()
    E = ops._ext()
    assert E is not None and E.abi_version() == 4
    assert hasattr(torch.ops.qqq_amd_native, "qqq_gemm") and hasattr(torch.ops.qqq_amd_native, "dynamic_quant")
    A = torch.zeros((4, 128), dtype=torch.int8)
    B = torch.zeros((8, 256), dtype=torch.int32)
    C = torch.zeros((1024, 128), dtype=torch.int32)
    D = torch.zeros((4, 128), dtype=torch.float16)
    s1, s2, s3 = torch.zeros((4, 1)), torch.zeros((1, 128)), torch.zeros(0, dtype=torch.float16)
    ws = torch.zeros(16, dtype=torch.int32)
    cases = [
        (dict(), "must live on the same GPU as A"),
        (dict(s1=s1.double()), "s1 dtype must be float32, but got"),
        (dict(ws=torch.zeros(3, dtype=torch.int32)), "workspace must be of size at least 16."),
        (dict(s3=torch.zeros((3, 128), dtype=torch.float16)), "k=128 not compatible with 3 groups."),
    ]
    for kw, msg in cases:
        args = dict(A=A, B=B, C=C, D=D, s1=s1, s2=s2, s3=s3, ws=ws)
        args.update(kw)
        for fn in (E.qqq_gemm, ops._qqq_gemm_impl):
            with pytest.raises(RuntimeError) as ei:
                fn(args["A"], args["B"], args["C"], args["D"], args["s1"], args["s2"], args["s3"], args["ws"], -1, -1, -1, 16)
            assert msg in str(ei.value), (fn, msg, str(ei.value)[:200])
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.dynamic_quant(torch.zeros((2, 64), dtype=torch.float16))


def test_uneven_k_slices_in_the_plan():
    """Round 5 (profiles/r05_uneven_k_slices.txt): with a split K the panel kernel gives its LAST slice `skew` stages more than an even share, so that it arrives
    last and finds the other deposits complete.  Automatic where measured: 4 stages at 128 tokens on the BASELINE layer (3 per-group, 3 in two slices), never so
    many that a slice keeps fewer than four stages, none without a split; tune.skew = -1 switches it off, a positive value pins it (clamped the same way)."""
    from qqq_amd import _lib

    N, K = 8192, 21760
    p = _lib.plan(128, N, K, -1, 16)
    assert (p["kernel"], p["ksplit"], p["skew"]) == (4, 4, 4), p
    assert _lib.plan(128, N, K, 128, 16)["skew"] == 3
    p = _lib.plan(256, N, K, -1, 16, tune=dict(kernel=4))   # 128-column strips, two m-blocks, two slices
    assert (p["kernel"], p["bm"], p["ksplit"], p["skew"]) == (4, 128, 2, 3), p
    assert _lib.plan(128, N, K, -1, 16, tune=dict(skew=-1))["skew"] == 0 and _lib.plan(128, N, K, -1, 16, tune=dict(skew=9))["skew"] == 9
    assert _lib.plan(128, N, K, -1, 16, tune=dict(kernel=4, ksplit=1))["skew"] == 0                     # nothing to hand off
    assert _lib.plan(128, N, K, -1, 16, have_scratch=False)["skew"] == 0
    # short K: 4096 x 4096 at 128 tokens = 32 stages in 4 slices -> at most 32 - 16 stages to give away; K = 2048: 16 stages, nothing
    p = _lib.plan(128, 4096, 4096, -1, 16, tune=dict(kernel=4, ksplit=4, skew=63))
    assert (p["ksplit"], p["skew"]) == (4, 16), p
    p = _lib.plan(128, 4096, 2048, -1, 16, tune=dict(kernel=4, ksplit=4, skew=5))
    assert p["skew"] == 0 and p["ksplit"] == 4, p
    # the slices as the kernel cuts them (qqq_panel.hip.h): every stage exactly once, the last slice the longest by `skew`
    for nst, ks, skew in ((170, 4, 4), (170, 2, 3), (32, 4, 3), (85, 3, 7), (171, 4, 0)):
        cuts = [(nst - skew) * sp // ks for sp in range(ks)] + [nst]
        lens = [cuts[i + 1] - cuts[i] for i in range(ks)]
        assert sum(lens) == nst and min(lens) >= 4 and lens[-1] - max(lens[:-1]) in (skew, skew - 1, skew + 1), (nst, ks, skew, lens)
    # the wide kernel's two-slice split takes the same knob: 256 KiB deposits, ~20 us from last MFMA to "complete" -> 6 stages per-group at 1024 tokens
    # (173.1 -> 165.9 us, profiles/r05_uneven_k_slices_wide.txt), 7 for the 256 x 128 tiles per-channel at 384 / 512 tokens
    p = _lib.plan(1024, N, K, 128, 16)
    assert (p["kernel"], p["ksplit"], p["skew"], p["fused"] & 64) == (5, 2, 7, 0), p  # (round 6, rates refitted on the rebuilt loop: the same hand-off time is 7 of its shorter stages)
    # (round 6: tune.fused bit 64 = two slices of 256-column tiles EXCHANGE row halves -- even slices, the plan's fused field carries the bit; measured level, not the default)
    p = _lib.plan(1024, N, K, 128, 16, tune=dict(fused=64))
    assert (p["kernel"], p["ksplit"], p["skew"], p["fused"] & 64) == (5, 2, 0, 64), p
    p = _lib.plan(1024, N, K, 128, 16, tune=dict(skew=5, fused=64))   # a pinned skew is the classic fold with uneven slices
    assert (p["skew"], p["fused"] & 64) == (5, 0), p
    assert _lib.plan(1024, N, K, 128, 16, tune=dict(skew=5))["skew"] == 5 and _lib.plan(1024, N, K, 128, 16, tune=dict(skew=-1))["skew"] == 0
    p = _lib.plan(512, N, K, -1, 16)
    assert (p["kernel"], p["bm"], p["ksplit"], p["skew"]) == (5, 128, 2, 7), p


def test_tiled_family_is_not_an_automatic_choice():
    """Round 5: the tiled family (round 1's kernel) never won one of the 903 measured dispatch points of round 4 and is no longer a candidate of the automatic
    dispatch; it stays reachable through tune.kernel = 2 (the fuzzers' independent reference)."""
    from qqq_amd import _lib

    for gs in (-1, 128):
        for (n, k) in ((8192, 21760), (4096, 4096), (11008, 4096), (4096, 11008), (1024, 8192), (28672, 8192), (3584, 18944), (5120, 13824)):
            for m in (1, 8, 16, 33, 64, 65, 128, 129, 256, 257, 384, 512, 768, 1024, 1536, 2048, 4096, 8192, 16384):
                assert _lib.plan(m, n, k, gs, 16)["kernel"] != 2, (m, n, k, gs)
    assert _lib.plan(4096, 8192, 21760, -1, 16, tune=dict(kernel=2))["kernel"] == 2


def test_column_kernel_takes_sixteen_waves_where_the_requantiser_binds():
    """Round 5: per-group up to 8 tokens the column kernel's workgroups have sixteen waves (-2 ... -6 % on five layer shapes, profiles/r05_column_16_waves.txt); per-channel
    and from 9 tokens eight; tune.waves = 16 forces it for one 16-token tile."""
    from qqq_amd import _lib

    N, K = 8192, 21760
    assert [_lib.plan(m, N, K, 128, 16)["waves"] for m in (1, 8)] == [16, 16] and _lib.plan(1, 4096, 4096, 128, 16)["waves"] == 16
    assert _lib.plan(1, N, K, -1, 16)["waves"] == 8 and _lib.plan(12, 4096, 4096, 128, 16)["waves"] == 8
    assert _lib.plan(4, N, K, -1, 16, tune=dict(kernel=3, waves=16))["waves"] == 16 and _lib.plan(24, N, K, -1, 16, tune=dict(kernel=3, mt=2, waves=16))["waves"] == 8


def test_panel_kernel_is_a_candidate_from_17_tokens():
    """Round 5 (cold grids): on very wide layers 256-column strips in two or three K slices beat column and stream kernel at 17 ... 32 tokens (N = 20480, K = 7168 at 32
    tokens: 21.7 us against 27.2 / 32.6); up to 16 tokens the choice stays between those two, and a tie between them goes to the column kernel (one launch)."""
    from qqq_amd import _lib

    p = _lib.plan(32, 20480, 7168, -1, 16)
    assert (p["kernel"], p["bm"]) == (4, 256) and p["ksplit"] in (2, 3), p
    assert _lib.plan(32, 28672, 8192, -1, 16)["kernel"] == 4
    assert _lib.plan(16, 20480, 7168, -1, 16)["kernel"] in (1, 3)
    assert _lib.plan(32, 4096, 4096, -1, 16)["kernel"] == 3 and _lib.plan(24, 8192, 8192, -1, 16)["kernel"] == 3
    assert _lib.plan(8, 8192, 21760, 128, 16)["kernel"] == 3  # (the tie: 25.6 vs 25.5 us modelled, 22.3 vs 24.2 measured)
    prices = _lib.model_us(24, 8192, 8192, -1, 16)
    assert set(prices) == {"column", "stream", "panel"} and all(v > 0 for v in prices.values()), prices


def test_plan_is_pure_host_logic_with_the_mi355x_cu_count():
    """qqq_w4a8_plan no longer asks the HIP runtime for the current device's CU count (the tile-walk decision depends on it); it plans for the
    MI355X's 256.  qqq_w4a8_gemm_ex plans and launches with the CU count of the device it was GIVEN, capped by `sms`."""
    from qqq_amd import _lib

    p = _lib.plan(8192, 4096, 4096, -1, 16)   # 512 tiles of 256 x 256 on 256 CUs, K = 4096: the persistent tile walk
    assert p["kernel"] == 5 and p["glds"] == 2, p
    p = _lib.plan(2048, 4096, 4096, -1, 16)   # 128 tiles: fewer than one per CU -> one tile per workgroup
    assert p["kernel"] == 5 and p["glds"] == 1, p


def test_planner_header_is_pure_host_code(tmp_path):
    """csrc/qqq_plan.h -- make_plan, the cost models, the M split -- compiles ALONE with the host compiler: no HIP header, no __global__, nothing of the
    kernels' translation unit.  That is what lets a planner change be compiled and compared (tools/plan_dump.py) without building a kernel; a HIP
    dependency that creeps in fails here."""
    import shutil
    import subprocess

    gxx = shutil.which("g++")
    assert gxx, "g++ not found: the planner header's host-purity check needs the host compiler"
    hdr = os.path.join(ROOT, "qqq_amd", "csrc", "qqq_plan.h")
    src = open(hdr).read() + open(os.path.join(ROOT, "qqq_amd", "csrc", "qqq_rates.h")).read()
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|__device__|#include\s*<hip", src)
    includes = set(re.findall(r'#include\s*([<"][^>"]+[>"])', open(hdr).read()))
    assert {i for i in includes if i.startswith('"')} == {'"../../include/qqq_amd.h"', '"qqq_rates.h"'}, includes
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-function", "-x", "c++", hdr], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
