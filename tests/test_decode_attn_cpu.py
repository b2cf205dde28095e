"""Split-K decode attention without a GPU: the C-ABI of include/qqq_amd_decode.h (declared set, export, argument checks before any launch,
workspace sizes), the kernels' resources in the gfx950 code object, and the modules' opt-in flag (state-dict, loading, no cycles)."""
import gc
import os
import sys
import weakref

import pytest
import torch

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
    names = _declared("qqq_amd_decode.h")
    assert names == {"qqq_decode_attn", "qqq_decode_attn_workspace_bytes"}
    for n in names:
        assert hasattr(L, n)
    assert L.qqq_amd_abi_version() == 4


# fake device addresses with the alignment the entry point asks for: the calls below must fail in the checks, before any launch
A16, A8, A4 = 0x10000, 0x20008, 0x30004
WS = 1 << 30


def _dec(L, q=A16, kc=A16, vc=A16, pos=A8, scale=0.088, o=A16, xq=A8, s1=A4, ws=A16, wsb=WS, b=2, h=32, kvh=8, d=128, cap=4096,
         max_len=4096):
    return L.qqq_decode_attn(q, kc, vc, pos, scale, o, xq, s1, ws, wsb, b, h, kvh, d, cap, max_len, 0, None)


BAD = [dict(q=None), dict(kc=None), dict(vc=None), dict(pos=None), dict(ws=None), dict(o=None, xq=None, s1=None), dict(xq=None),
       dict(s1=None), dict(q=A16 + 8), dict(kc=A16 + 2), dict(vc=A16 + 4), dict(pos=A8 + 4), dict(o=A16 + 8), dict(xq=A8 + 4),
       dict(s1=A4 + 2), dict(ws=A16 + 8), dict(wsb=0), dict(wsb=1000), dict(d=96), dict(d=256), dict(d=32), dict(d=0), dict(h=30),
       dict(h=72), dict(h=0), dict(kvh=0), dict(h=256, kvh=32), dict(b=-1), dict(h=-32), dict(kvh=-8), dict(d=-128), dict(cap=-1),
       dict(max_len=-1), dict(max_len=0), dict(max_len=4097), dict(cap=0, max_len=0), dict(b=65536)]


@pytest.mark.parametrize("kw", BAD)
def test_decode_attn_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _dec(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_decode_attn:")


def test_workspace_check_uses_the_workspace_size(L):
    from qqq_amd import _lib

    need = L.qqq_decode_attn_workspace_bytes(2, 32, 8, 128, 4096)
    assert need > 0
    assert _dec(L, wsb=need - 1) == ERR_ARG and "workspace" in _lib.last_error()


def test_b0_is_a_no_op(L):
    assert _dec(L, b=0) == 0
    assert L.qqq_decode_attn(None, None, None, None, 1.0, None, None, None, None, 0, 0, 32, 8, 128, 4096, 4096, 0, None) == 0
    assert L.qqq_decode_attn_workspace_bytes(0, 32, 8, 128, 4096) == 0


def test_workspace_sizes_are_monotone_in_max_len(L):
    for b, h, kvh, d in ((1, 32, 32, 128), (16, 32, 8, 128), (4, 14, 2, 64), (3, 28, 4, 128)):
        sizes = [L.qqq_decode_attn_workspace_bytes(b, h, kvh, d, n) for n in range(1, 20000, 37)]
        assert all(s > 0 for s in sizes) and all(a <= c for a, c in zip(sizes, sizes[1:])), (b, h, kvh, d)
        assert L.qqq_decode_attn_workspace_bytes(b, h, kvh, d, 1 << 20) <= b * h * 32 * (d + 2) * 4  # bounded split count
    assert L.qqq_decode_attn_workspace_bytes(1, 32, 8, 96, 4096) == 0 and L.qqq_decode_attn_workspace_bytes(1, 72, 8, 128, 4096) == 0


def test_decode_kernels_in_the_code_object_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB) if k["demangled"].startswith("qqq_decode_")}
    assert set(ks) == {"qqq_decode_split_kernel<64>", "qqq_decode_split_kernel<128>", "qqq_decode_combine_kernel<1,512>",
                       "qqq_decode_combine_kernel<2,512>", "qqq_decode_combine_kernel<4,512>"}
    for k in ks.values():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    for d in (64, 128):
        k = ks[f"qqq_decode_split_kernel<{d}>"]
        assert k["max_flat_workgroup_size"] == 256 and k["vgpr_count"] + k["agpr_count"] <= 128, k  # four waves per SIMD
        assert k["group_segment_fixed_size"] <= 4 * 8 * d * 4 + 256, k  # LDS: the four waves' partials only


def test_cpu_tensors_raise():
    from qqq_amd import ops

    q = torch.zeros((1, 4, 1, 64), dtype=torch.float16)
    cache = torch.zeros((1, 2, 16, 64), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.decode_attention(q, cache, cache.clone(), torch.zeros(1, dtype=torch.int64), 0.125)
    from qqq_amd import KVCache, QuantLlamaAttention

    attn = QuantLlamaAttention(256, 4, 2, -1).fuse_decode()
    with pytest.raises(RuntimeError, match="no CPU path"):
        attn(torch.zeros((1, 1, 256), dtype=torch.float16), KVCache(1, 1, 2, 64, 16), 3)


def test_fuse_decode_keeps_the_state_dict_and_survives_loading_and_moves():
    from qqq_amd import QuantLlamaDecoderLayer

    layer = QuantLlamaDecoderLayer(256, 4, 2, 512, 128)
    keys = set(layer.state_dict())
    sd = {k: v.clone() for k, v in layer.state_dict().items()}
    assert not layer.decode_fused
    assert layer.fuse_decode() is layer and layer.decode_fused and layer.self_attn.decode_fused
    assert set(layer.state_dict()) == keys
    layer.load_state_dict(sd, strict=True)
    assert layer.decode_fused
    layer.to(torch.float32).to(torch.float16)
    assert layer.decode_fused
    assert layer.self_attn.unfuse_decode() is layer.self_attn and not layer.decode_fused
    assert layer.unfuse_decode() is layer and not layer.decode_fused


def test_layer_is_freed_without_the_cycle_collector():
    from qqq_amd import QuantLlamaDecoderLayer

    gc.collect()
    gc.disable()
    try:
        layer = QuantLlamaDecoderLayer(256, 4, 2, 512, 128).fuse_decode()
        layer.self_attn.fuse_qkv()
        ref = weakref.ref(layer)
        attn = weakref.ref(layer.self_attn)
        del layer
        assert ref() is None and attn() is None
    finally:
        gc.enable()
