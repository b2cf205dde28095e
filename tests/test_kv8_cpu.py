"""The int8 KV cache without a GPU: the C-ABI of include/qqq_amd_kv8.h (declared set, exports, argument checks before any launch), the two
kernels' resources in the gfx950 code object, the ops' CPU refusal, and KVCache(dtype=torch.int8): layout, nbytes, dequant."""
import os
import sys

import pytest
import torch

import kv8_ref as K8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 17


@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def test_header_declares_the_two_functions_and_the_library_exports_them(L):
    from qqq_amd import _abi

    names = set(_abi.prototypes(os.path.join(ROOT, "include", "qqq_amd_kv8.h")))
    assert names == {"qqq_rope_qkv_kv8", "qqq_decode_attn_kv8"}
    for n in names:
        assert hasattr(L, n)
    assert L.qqq_amd_abi_version() == 4


# fake device addresses with the alignment the entry points ask for: the calls below must fail in the checks, before any launch
A16, A8, A4 = 0x10000, 0x20008, 0x30004
WS = 1 << 30


def _rope(L, q=A16, ld_q=None, k=A16, ld_k=None, v=A16, ld_v=None, cos=A16, sin=A16, table_len=4096, pos=A8, q_out=A16, kc=A16, vc=A16,
          ks=A4, vs=A4, b=2, s=3, h=32, kvh=8, d=128, cap=4096):
    ld_q = h * d if ld_q is None else ld_q
    ld_k = kvh * d if ld_k is None else ld_k
    ld_v = kvh * d if ld_v is None else ld_v
    return L.qqq_rope_qkv_kv8(q, ld_q, k, ld_k, v, ld_v, cos, sin, table_len, pos, q_out, kc, vc, ks, vs, b, s, h, kvh, d, cap, 0, None)


ROPE_BAD = [dict(ks=None), dict(vs=None), dict(kc=None), dict(vc=None), dict(q=None), dict(pos=None), dict(q_out=None), dict(d=96),
            dict(d=32), dict(d=256), dict(d=16), dict(h=30), dict(kvh=0), dict(kc=A16 + 8), dict(vc=A16 + 4),
            dict(ks=A4 + 2), dict(vs=A4 + 1), dict(q=A16 + 8), dict(pos=A8 + 4), dict(q_out=A16 + 2), dict(ld_q=4095), dict(ld_k=1028),
            dict(b=-1), dict(cap=-1), dict(table_len=-1)]


@pytest.mark.parametrize("kw", ROPE_BAD)
def test_rope_qkv_kv8_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _rope(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_rope_qkv_kv8:")


def _dec(L, q=A16, kc=A16, vc=A16, ks=A4, vs=A4, pos=A8, scale=0.088, o=A16, xq=A8, s1=A4, ws=A16, wsb=WS, b=2, h=32, kvh=8, d=128,
         cap=4096, max_len=4096):
    return L.qqq_decode_attn_kv8(q, kc, vc, ks, vs, pos, scale, o, xq, s1, ws, wsb, b, h, kvh, d, cap, max_len, 0, None)


DEC_BAD = [dict(ks=None), dict(vs=None), dict(q=None), dict(kc=None), dict(vc=None), dict(pos=None), dict(ws=None),
           dict(o=None, xq=None, s1=None), dict(xq=None), dict(s1=None), dict(d=96), dict(d=256), dict(d=32), dict(h=72), dict(h=30),
           dict(h=0), dict(kvh=0), dict(h=256, kvh=32), dict(q=A16 + 8), dict(kc=A16 + 2), dict(vc=A16 + 4), dict(ks=A4 + 2),
           dict(vs=A4 + 1), dict(pos=A8 + 4), dict(o=A16 + 8), dict(xq=A8 + 4), dict(s1=A4 + 2), dict(ws=A16 + 8), dict(wsb=0),
           dict(wsb=1000), dict(max_len=0), dict(max_len=-1), dict(max_len=4097), dict(cap=0, max_len=0), dict(b=-1), dict(b=65536)]


@pytest.mark.parametrize("kw", DEC_BAD)
def test_decode_attn_kv8_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _dec(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_decode_attn_kv8:")


def test_workspace_check_uses_the_fp16_kernels_workspace_size(L):
    from qqq_amd import _lib

    need = L.qqq_decode_attn_workspace_bytes(2, 32, 8, 128, 4096)
    assert need > 0
    assert _dec(L, wsb=need - 1) == ERR_ARG and "workspace" in _lib.last_error()


def test_b0_is_a_no_op(L):
    assert _dec(L, b=0) == 0
    assert L.qqq_decode_attn_kv8(None, None, None, None, None, None, 1.0, None, None, None, None, 0, 0, 32, 8, 128, 4096, 4096, 0, None) == 0
    assert _rope(L, b=0) == 0 and _rope(L, s=0) == 0
    assert L.qqq_rope_qkv_kv8(None, 0, None, 0, None, 0, None, None, 0, None, None, None, None, None, None, 0, 1, 32, 8, 128, 64, 0,
                              None) == 0


def test_kv8_kernels_in_the_code_object_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB) if k["demangled"].startswith("qqq_kv8_")}
    assert set(ks) == {"qqq_kv8_rope_qkv_kernel<128>", "qqq_kv8_decode_split_kernel<64>", "qqq_kv8_decode_split_kernel<128>"}
    for k in ks.values():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    rope = ks["qqq_kv8_rope_qkv_kernel<128>"]
    assert rope["group_segment_fixed_size"] == 0 and rope["max_flat_workgroup_size"] == 128, rope  # the amax crosses lanes, not LDS
    for d in (64, 128):
        k = ks[f"qqq_kv8_decode_split_kernel<{d}>"]
        assert k["max_flat_workgroup_size"] == 256 and k["vgpr_count"] + k["agpr_count"] <= 128, k  # four waves per SIMD
        assert k["group_segment_fixed_size"] <= 4 * 8 * d * 4 + 256, k  # LDS: the four waves' partials only


def test_cpu_tensors_raise():
    from qqq_amd import KVCache, QuantLlamaAttention, ops

    d = 64
    q = torch.zeros((1, 4, 1, d), dtype=torch.float16)
    kc, sc = torch.zeros((1, 2, 16, d), dtype=torch.int8), torch.zeros((1, 2, 16), dtype=torch.float32)
    pos = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.decode_attention_kv8(q, kc, kc.clone(), sc, sc.clone(), pos, 0.125)
    rows = torch.zeros((1, 4 * d), dtype=torch.float16)
    kv = torch.zeros((1, 2 * d), dtype=torch.float16)
    tab = torch.zeros((16, d), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rope_qkv_kv8(rows, kv, kv.clone(), tab, tab.clone(), pos, kc, kc.clone(), sc, sc.clone())
    attn = QuantLlamaAttention(256, 4, 2, -1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        attn(torch.zeros((1, 1, 256), dtype=torch.float16), KVCache(1, 1, 2, 64, 16, dtype=torch.int8), 3)


def test_int8_cache_refuses_head_shapes_the_decode_kernel_does_not_take():
    from qqq_amd import KVCache, QuantLlamaAttention

    attn = QuantLlamaAttention(256, 8, 2, -1)  # head_dim 32
    xq, s1 = torch.zeros((1, 256), dtype=torch.int8), torch.zeros((1, 1), dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="int8 KV cache"):
        attn.forward_int8(xq, s1, KVCache(1, 1, 2, 32, 16, dtype=torch.int8), 0)


def test_int8_kvcache_layout_nbytes_and_dequant():
    from qqq_amd import KVCache

    L_, b, kvh, d, cap = 3, 2, 4, 128, 40
    c = KVCache(L_, b, kvh, d, cap, dtype=torch.int8)
    assert c.dtype == torch.int8 and c.quantized
    assert len(c.k) == len(c.v) == len(c.k_scale) == len(c.v_scale) == L_
    for t in c.k + c.v:
        assert t.dtype == torch.int8 and t.shape == (b, kvh, cap, d) and t.is_contiguous() and not t.any()
    for t in c.k_scale + c.v_scale:
        assert t.dtype == torch.float32 and t.shape == (b, kvh, cap) and t.is_contiguous() and not t.any()
    assert c.nbytes == 2 * L_ * b * kvh * cap * (d + 4)
    assert c.nbytes == sum(t.numel() * t.element_size() for t in c.k + c.v + c.k_scale + c.v_scale)
    assert torch.equal(c.positions(5, 1), torch.tensor([5, 5])) and torch.equal(c.positions(3, 2), torch.tensor([3, 4, 3, 4]))
    g = torch.Generator().manual_seed(1)
    x = (torch.randn((b, kvh, cap, d), generator=g) * torch.rand((b, kvh, cap, 1), generator=g) * 8).half()
    x[0, 0, 3] = 0  # an all-zero row: zero codes, zero scale
    y = torch.randn((b, kvh, cap, d), generator=g).half()
    c.k[1], c.k_scale[1] = K8.quant_rows(x)
    c.v[1], c.v_scale[1] = K8.quant_rows(y)
    for length in (1, 17, cap):
        kd, vd = c.dequant(1, length)
        for got, codes, sc, src in ((kd, c.k[1], c.k_scale[1], x), (vd, c.v[1], c.v_scale[1], y)):
            assert got.dtype == torch.float16 and got.shape == (b, kvh, length, d)
            want = K8.dequant64(codes[:, :, :length], sc[:, :, :length])
            assert torch.equal(got, want.half())  # fp16(float(code) * scale): the fp32 product is exact
            # half a quantisation step per element: |x - code * s| <= s / 2, plus the fp16 rounding of the product
            step = sc[:, :, :length, None].double()
            assert bool(((got.double() - src[:, :, :length].double()).abs() <= 0.5 * step + 2.0 ** -11 * want.abs() + 1e-12).all())
    assert not c.dequant(1, cap)[0][0, 0, 3].any()


def test_default_kvcache_is_unchanged_and_other_dtypes_raise():
    from qqq_amd import KVCache

    c = KVCache(2, 3, 4, 64, 20)
    assert c.dtype == torch.float16 and not c.quantized and not hasattr(c, "k_scale") and not hasattr(c, "v_scale")
    assert all(t.dtype == torch.float16 and t.shape == (3, 4, 20, 64) for t in c.k + c.v)
    assert c.nbytes == 4 * 2 * 3 * 4 * 20 * 64
    assert torch.equal(c.positions(7, 1), torch.tensor([7, 7, 7])) and torch.equal(c.positions(2, 2), torch.tensor([2, 3, 2, 3, 2, 3]))
    with pytest.raises(RuntimeError, match="not int8"):
        c.dequant(0, 4)
    for dt in (torch.bfloat16, torch.float32, torch.uint8, torch.float8_e4m3fn):
        with pytest.raises(ValueError, match="dtype"):
            KVCache(1, 1, 1, 64, 8, dtype=dt)
