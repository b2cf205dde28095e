"""Decoder-block activation quantisers without a GPU: the C-ABI of include/qqq_amd_act.h (declared set, exports, argument checks before
any launch), the kernels' resources in the gfx950 code object, the modules' reference-keyed state-dicts, and the numpy restatement."""
import os
import sys

import numpy as np
import pytest
import torch

import act_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 17


@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def _declared(header):
    from qqq_amd import _abi

    return set(_abi.prototypes(os.path.join(ROOT, "include", header)))


def test_header_declares_the_two_functions_and_the_library_exports_them(L):
    names = _declared("qqq_amd_act.h")
    assert names == {"qqq_rmsnorm_quant", "qqq_silu_mul_quant"}
    for n in names:
        assert hasattr(L, n), n
    assert L.qqq_amd_abi_version() == 4


# fake device addresses with the alignment the entry points ask for (16 / 8 / 4 bytes): the calls below must fail in the checks
A16, A8, A4 = 0x1000, 0x2008, 0x3004


def _rms(L, x=A16, r=None, w=A16, y=None, xq=A8, s1=A4, m=4, k=64):
    return L.qqq_rmsnorm_quant(x, r, w, 1e-6, y, xq, s1, m, k, 0, None)


def _silu(L, g=A16, ldg=64, u=A16, ldu=64, y=None, xq=A8, s1=A4, m=4, i=64):
    return L.qqq_silu_mul_quant(g, ldg, u, ldu, y, xq, s1, m, i, 0, None)


@pytest.mark.parametrize("kw", [dict(x=None), dict(w=None), dict(xq=None), dict(s1=None), dict(k=12), dict(k=65544), dict(m=-1),
                                dict(k=-8), dict(x=A16 + 8), dict(w=A16 + 2), dict(r=A16 + 8), dict(y=A16 + 4), dict(xq=A8 + 4),
                                dict(s1=A4 + 2)])
def test_rmsnorm_quant_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _rms(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_rmsnorm_quant:")


@pytest.mark.parametrize("kw", [dict(g=None), dict(u=None), dict(xq=None), dict(s1=None), dict(i=12, ldg=16, ldu=16),
                                dict(i=65544, ldg=65544, ldu=65544), dict(ldg=56), dict(ldu=32), dict(ldg=68), dict(ldu=100),
                                dict(g=A16 + 8), dict(u=A16 + 2), dict(y=A16 + 8), dict(xq=A8 + 1), dict(s1=A4 + 1), dict(m=-2)])
def test_silu_mul_quant_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _silu(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_silu_mul_quant:")


def test_empty_problems_are_no_ops(L):
    # nothing is dereferenced, nothing is launched: NULL pointers are fine for m = 0 or k = 0
    assert L.qqq_rmsnorm_quant(None, None, None, 1e-6, None, None, None, 0, 4096, 0, None) == 0
    assert L.qqq_rmsnorm_quant(None, None, None, 1e-6, None, None, None, 16, 0, 0, None) == 0
    assert L.qqq_silu_mul_quant(None, 0, None, 0, None, None, None, 0, 11008, 0, None) == 0
    assert L.qqq_silu_mul_quant(None, 0, None, 0, None, None, None, 3, 0, 0, None) == 0


def test_kernels_in_the_code_object_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB)}
    for fam in ("qqq_rmsnorm_quant_kernel", "qqq_silu_mul_quant_kernel"):
        # the launch shapes of the host dispatch (qqq_w4a8.hip: act_launch, the one ladder of the three per-row quantisers)
        for vpt, nt in ((2, 256), (4, 256), (8, 256), (2, 1024), (4, 1024), (8, 1024)):
            k = ks[f"{fam}<{vpt},{nt}>"]
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
            assert k["max_flat_workgroup_size"] == nt


def test_cpu_tensors_raise():
    from qqq_amd import ops

    x = torch.zeros((2, 64), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rmsnorm_quant(x, torch.ones(64, dtype=torch.float16), 1e-6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.silu_mul_quant(x, x)


def test_modules_load_reference_keyed_state_dicts_strictly():
    from qqq_amd import QuantLinear, QuantLlamaMLP, QuantRMSNorm

    hidden, inter = 256, 512
    for gs in (-1, 128):
        # the reference module's keys: QuantizedLlamaMLP = gate_proj / up_proj / down_proj QuantLinears (bias=False)
        ref = torch.nn.Module()
        ref.gate_proj = QuantLinear(4, gs, hidden, inter, bias=False)
        ref.up_proj = QuantLinear(4, gs, hidden, inter, bias=False)
        ref.down_proj = QuantLinear(4, gs, inter, hidden, bias=False)
        g = torch.Generator().manual_seed(1)
        sd = {k: (torch.randint(-2**31, 2**31 - 1, v.shape, generator=g, dtype=torch.int32) if v.dtype == torch.int32
                  else torch.rand(v.shape, generator=g).to(v.dtype)) for k, v in ref.state_dict().items()}
        mlp = QuantLlamaMLP(hidden, inter, gs)
        assert set(mlp.state_dict()) == set(sd)
        mlp.load_state_dict(sd, strict=True)
        for k, v in mlp.state_dict().items():
            assert torch.equal(v, sd[k]), k
    norm = QuantRMSNorm(hidden, eps=1e-5)
    w = torch.rand(hidden)  # LlamaRMSNorm's weight: a float parameter named `weight`
    norm.load_state_dict({"weight": w}, strict=True)
    assert norm.weight.dtype == torch.float16 and torch.equal(norm.weight, w.half())


def test_fuse_gate_up_needs_no_gpu_and_leaves_the_state_dict_alone():
    from qqq_amd import QuantLlamaMLP

    mlp = QuantLlamaMLP(128, 256, -1)
    for i, t in enumerate(mlp.state_dict().values()):  # defined contents (torch.empty may hold NaN bit patterns)
        t.copy_(torch.arange(t.numel()).reshape(t.shape) + i)
    before = {k: v.clone() for k, v in mlp.state_dict().items()}
    mlp.fuse_gate_up()
    assert mlp.gate_up_fused
    fused = mlp._gate_up
    assert fused.outfeatures == 512 and torch.equal(fused.B, torch.cat([mlp.gate_proj.B, mlp.up_proj.B], 1))
    # a second copy of gate/up's weights, outside the state-dict
    assert fused.B.numel() == mlp.gate_proj.B.numel() + mlp.up_proj.B.numel()
    assert fused.B.data_ptr() not in {t.data_ptr() for t in mlp.state_dict().values()}
    sd = mlp.state_dict()
    assert set(sd) == set(before) and all(torch.equal(sd[k], before[k]) for k in sd)
    mlp.load_state_dict(before, strict=True)  # loading drops the (possibly stale) fused copy
    assert not mlp.gate_up_fused


def test_mlp_is_freed_without_the_cycle_collector():
    import gc
    import weakref

    from qqq_amd import QuantLlamaMLP

    gc.collect()
    gc.disable()
    try:
        mlp = QuantLlamaMLP(128, 256, 128).fuse_gate_up()
        ref = weakref.ref(mlp)
        del mlp
        assert ref() is None  # no reference cycle: the weights (on the GPU, device memory) go with the last reference
    finally:
        gc.enable()


def test_quant_rows_matches_the_c_oracle():
    from oracle import c_oracle as C

    rng = np.random.default_rng(3)
    for m, k in ((1, 8), (5, 4096), (9, 11008)):
        y = (rng.standard_normal((m, k)) * 2.3).astype(np.float16)
        y[0] = 0
        if m > 2:
            y[1, k // 2] = 60000
            y[2] = (rng.random(k) * 2 - 1) * 65000
        q, s = R.quant_rows(y)
        oq, os_ = C.dynamic_quant(y, "recip")
        assert np.array_equal(q, oq) and np.array_equal(s.view(np.uint32), os_.view(np.uint32)), (m, k)
        assert not q[0].any() and s[0, 0] == 0


def test_restatement_matches_numpy_in_float64_and_torch_cpu():
    rng = np.random.default_rng(4)
    m, k = 6, 4096
    x = (rng.standard_normal((m, k)) * 3).astype(np.float16)
    r = (rng.standard_normal((m, k)) * 3).astype(np.float16)
    w = (1 + 0.2 * rng.standard_normal(k)).astype(np.float16)
    x[0] = (rng.random(k) * 2 - 1) * 65000  # near fp16 max: fp32 squares do not overflow
    y, h = R.rmsnorm(x, w, 1e-6)
    h64 = x.astype(np.float64)
    n64 = h64 / np.sqrt((h64 ** 2).mean(1, keepdims=True) + 1e-6)
    assert np.isfinite(y).all()
    assert np.allclose(y.astype(np.float64), n64.astype(np.float16).astype(np.float64) * w, rtol=2e-3, atol=1e-4)
    y2, h2 = R.rmsnorm(x, w, 1e-6, residual=r)
    assert np.array_equal(h2, (torch.from_numpy(r) + torch.from_numpy(x)).numpy())  # torch's fp16 `+`
    ty, tn, _ = R.torch_rmsnorm(torch.from_numpy(x), torch.from_numpy(w), 1e-6)
    assert int(R.ulp_diff(torch.from_numpy(y), ty).max()) <= 2
    g = (rng.standard_normal((m, k)) * 4).astype(np.float16)
    g[0, :4] = (-65000, 65000, -20, 20)
    u = rng.standard_normal((m, k)).astype(np.float16)
    s = R.silu_mul(g, u)
    g64 = g.astype(np.float64)
    with np.errstate(over="ignore"):
        ref = (g64 / (1 + np.exp(-g64))).astype(np.float16).astype(np.float64) * u
    assert np.allclose(s.astype(np.float64), ref, rtol=2e-3, atol=1e-6)
    assert int(R.ulp_diff(torch.from_numpy(s), R.torch_silu_mul(torch.from_numpy(g), torch.from_numpy(u))).max()) <= 1


def test_ordered_round_trip():
    v = torch.tensor([-65504, -1.5, -0.0, 0.0, 6e-8, 1.0, 65504, float("inf")], dtype=torch.float16)
    o = R.ordered(v)
    assert torch.equal(R.from_ordered(o).view(torch.int16)[[0, 1, 3, 4, 5, 6, 7]], v.view(torch.int16)[[0, 1, 3, 4, 5, 6, 7]])
    assert torch.equal(R.from_ordered(o + 1)[4:7], torch.tensor([1.1920929e-07, 1.0009765625, float("inf")], dtype=torch.float16))
