"""The fused token sampler without a GPU: the C-ABI of include/qqq_amd_sample.h (declared set, exports, argument checks before any launch,
the NULL no-op), the qqq_sample_* kernel's resources in the gfx950 code object, the op's CPU refusal and fake implementation, and
tests/sample_ref.py against transformers' logits warpers."""
import os
import sys

import numpy as np
import pytest
import torch

from sample_ref import sample_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 17
ENTRIES = {"qqq_sample_tokens"}


@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def test_header_declares_the_entry_and_the_library_exports_it(L):
    from qqq_amd import _abi

    names = set(_abi.prototypes(os.path.join(ROOT, "include", "qqq_amd_sample.h")))
    assert names == ENTRIES
    for n in names:
        assert hasattr(L, n), n
    assert L.qqq_amd_abi_version() == 4
    main = _abi.source(os.path.join(ROOT, "include", "qqq_amd.h"))
    assert "qqq_sample" not in main  # the feature has its own header


# fake device addresses with the alignment the entry point asks for: the calls below must fail in the checks, before any launch
A16, A8, A4 = 0x10000, 0x20008, 0x30004


def _call(L, logits=A16, ld=32000, T=A4, k=A4, p=A4, u=A4, tokens=A8, rows=4, vocab=32000):
    return L.qqq_sample_tokens(logits, ld, T, k, p, u, tokens, rows, vocab, 0, None)


BAD = [dict(logits=None), dict(T=None), dict(k=None), dict(p=None), dict(u=None), dict(tokens=None), dict(logits=A16 + 8), dict(logits=A16 + 2),
       dict(T=A4 + 2), dict(k=A4 + 1), dict(p=A4 + 2), dict(u=A4 + 3), dict(tokens=A8 + 4), dict(ld=31999), dict(ld=31992),
       dict(vocab=1001, ld=1001), dict(vocab=1001, ld=1004), dict(vocab=1001, ld=1000), dict(vocab=0, ld=8), dict(vocab=0, ld=0),
       dict(vocab=-1, ld=8), dict(vocab=262145, ld=262152), dict(rows=-1), dict(rows=65536)]


@pytest.mark.parametrize("kw", BAD)
def test_sample_tokens_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _call(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_sample_tokens:")


def test_rows_0_is_a_no_op_with_null_pointers(L):
    z = None
    assert L.qqq_sample_tokens(z, 0, z, z, z, z, z, 0, 32000, 0, z) == 0
    assert L.qqq_sample_tokens(z, 0, z, z, z, z, z, 0, 0, 0, z) == 0
    assert _call(L, rows=0) == 0


def test_sample_kernel_in_the_code_object_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB) if k["demangled"].startswith("qqq_sample_")}
    assert set(ks) == {"qqq_sample_tokens_kernel"}
    for k in ks.values():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        # sixteen waves; registers and LDS leave room for two workgroups per CU (128 registers per lane, 80 KB each)
        assert k["max_flat_workgroup_size"] == 1024 and k["vgpr_count"] + k["agpr_count"] <= 128 and k["group_segment_fixed_size"] <= 80 * 1024, k
    assert not any("sample" in k["demangled"] for k in code_object.kernels(build.LIB) if not k["demangled"].startswith("qqq_sample_"))


def test_cpu_tensors_raise():
    import qqq_amd
    from qqq_amd import ops

    assert qqq_amd.sample_tokens is ops.sample_tokens
    logits = torch.zeros((3, 40), dtype=torch.float16)
    u = torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sample_tokens(logits, 1.0, 0, 1.0, u)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sample_tokens(logits, torch.ones(3), torch.zeros(3, dtype=torch.int32), torch.ones(3), u)
    with pytest.raises(RuntimeError, match="temperature holds 2 entries"):
        ops.sample_tokens(logits, torch.ones(2), 0, 1.0, u)
    with pytest.raises(RuntimeError, match=r"fp16 \[rows, vocab\]"):
        ops.sample_tokens(logits[0], 1.0, 0, 1.0, u)


def test_fake_implementation_gives_int64_rows():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from qqq_amd import ops

    with FakeTensorMode():
        logits = torch.empty((9, 32000), dtype=torch.float16)
        f32, i32 = torch.empty(9), torch.empty(9, dtype=torch.int32)
        for out in (torch.ops.qqq_amd.sample_tokens(logits, f32, i32, f32, f32), ops.sample_tokens(logits, f32, i32, f32, f32)):
            assert out.shape == (9,) and out.dtype == torch.int64


def test_reference_greedy_and_special_values():
    l = np.array([0.5, 2.0, -np.inf, 2.0, np.nan], np.float16)
    for T, k in ((0.0, 0), (-1.0, 0), (float("nan"), 0), (1.0, 1)):
        r = sample_row(l, T, k, 1.0, 0.9)
        assert r["greedy"] and r["token"] == 1
    assert sample_row(l, 1.0, 0, 0.0, 0.0)["survive"].tolist() == [False, True, False, True, False]
    assert sample_row(l, 1.0, 0, 0.0, 0.0)["token"] == 1 and sample_row(l, 1.0, 0, 0.0, 0.99)["token"] == 3
    assert sample_row(l, 1.0, 2, 1.0, 0.0)["survive"].sum() == 2 and sample_row(l, 1.0, 3, 1.0, 0.0)["survive"].sum() == 3
    assert sample_row(np.full(5, -np.inf, np.float16), 1.0, 0, 1.0, 0.5)["token"] == 0
    assert sample_row(np.full(5, np.nan, np.float16), 1.0, 0, 1.0, 0.5)["token"] == 0
    for u in (1.5, np.nextafter(np.float32(1), np.float32(0))):
        assert sample_row(l, 1.0, 0, 1.0, u)["token"] == 3
    assert sample_row(l, 1.0, 0, 1.0, -1.0)["token"] == 0
    # ties at the k-th value are all kept
    assert sample_row(np.array([1, 3, 2, 2, 0], np.float16), 1.0, 2, 1.0, 0.0)["survive"].tolist() == [False, True, True, True, False]


@pytest.mark.parametrize("T", [0.5, 1.0, 1.7])
@pytest.mark.parametrize("k", [0, 5, 40])
@pytest.mark.parametrize("p", [1.0, 0.9, 0.5, 0.1])
def test_reference_surviving_set_equals_transformers_warpers_on_tie_free_logits(T, k, p):
    tr = pytest.importorskip("transformers")
    rng = np.random.default_rng(17)
    vocab = 200
    l = rng.permutation(np.linspace(-6.0, 6.0, vocab)).astype(np.float16)  # tie-free: distinct fp16 values
    assert np.unique(l).size == vocab
    scores = torch.from_numpy(l.astype(np.float32))[None]
    ids = torch.zeros((1, 1), dtype=torch.int64)
    scores = tr.TemperatureLogitsWarper(T)(ids, scores)
    if k > 0:
        scores = tr.TopKLogitsWarper(k)(ids, scores)
    if p < 1.0:
        scores = tr.TopPLogitsWarper(p)(ids, scores)
    want = torch.isfinite(scores[0]).numpy()
    # the warper compares f32 cumulative probabilities with 1 - p: stay clear of a cut within f32 rounding of an edge
    w = np.exp((l.astype(np.float64) - l.max()) / T) * sample_row(l, T, k, 1.0, 0.0)["survive"]
    cum = np.cumsum(np.sort(w)) / w.sum()
    assert np.abs(cum - (1.0 - p)).min() > 1e-5 or p == 1.0
    assert sample_row(l, T, k, p, 0.0)["survive"].tolist() == want.tolist()
