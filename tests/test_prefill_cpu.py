"""The paged prefill attention without a GPU: the C-ABI of include/qqq_amd_prefill.h (declared set, exports, argument checks before any
launch, the workspace, the NULL no-ops), the qqq_prefill_* kernels' resources in the gfx950 code object, the ops' CPU refusal and fake
implementations, PagedStep.cu_tokens / start_pos, and fuse_prefill() on the module."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 17
ENTRIES = {"qqq_prefill_attn_paged", "qqq_prefill_attn_paged_kv8", "qqq_prefill_attn_workspace_bytes"}


@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def test_header_declares_the_three_functions_and_the_library_exports_them(L):
    from qqq_amd import _abi

    names = set(_abi.prototypes(os.path.join(ROOT, "include", "qqq_amd_prefill.h")))
    assert names == ENTRIES
    for n in names:
        assert hasattr(L, n), n
    assert L.qqq_amd_abi_version() == 4


# fake device addresses with the alignment the entry points ask for: the calls below must fail in the checks, before any launch
A16, A8, A4 = 0x10000, 0x20008, 0x30004
WS = 1 << 30


def _pre(L, kv8, q=A16, kp=A16, vp=A16, ks=A4, vs=A4, table=A4, stride=32, cu=A4, sp=A8, scale=0.088, o=A16, xq=A8, s1=A4, ws=A16, wsb=WS,
         m=40, b=3, h=32, kvh=8, d=128, nb=64, bs=128, max_len=4096):
    tail = (table, stride, cu, sp, scale, o, xq, s1, ws, wsb, m, b, h, kvh, d, nb, bs, max_len, 0, None)
    return L.qqq_prefill_attn_paged_kv8(q, kp, vp, ks, vs, *tail) if kv8 else L.qqq_prefill_attn_paged(q, kp, vp, *tail)


BAD = [dict(q=None), dict(kp=None), dict(vp=None), dict(table=None), dict(cu=None), dict(sp=None), dict(o=None, xq=None, s1=None),
       dict(xq=None), dict(s1=None), dict(o=None, ws=None), dict(d=96), dict(d=256), dict(d=32), dict(h=72), dict(h=30), dict(h=0),
       dict(kvh=0), dict(h=256, kvh=32), dict(q=A16 + 8), dict(kp=A16 + 2), dict(vp=A16 + 4), dict(table=A4 + 2), dict(table=A4 + 1),
       dict(cu=A4 + 2), dict(cu=A4 + 1), dict(sp=A8 + 4), dict(o=A16 + 8), dict(xq=A8 + 4), dict(s1=A4 + 2), dict(ws=A16 + 8),
       dict(o=None, wsb=0), dict(o=None, wsb=1000), dict(max_len=0), dict(max_len=-1), dict(max_len=4097), dict(stride=31),
       dict(stride=0, max_len=1), dict(stride=-1), dict(m=-1), dict(b=-1), dict(b=65536), dict(bs=8, stride=512), dict(bs=24, stride=512),
       dict(bs=512, stride=512), dict(nb=0), dict(nb=-1), dict(nb=1 << 24, bs=256)]
BAD_KV8 = [dict(ks=None), dict(vs=None), dict(ks=A4 + 2), dict(vs=A4 + 1)]


@pytest.mark.parametrize("kv8,kw", [(False, kw) for kw in BAD] + [(True, kw) for kw in BAD + BAD_KV8])
def test_prefill_attn_paged_rejects_bad_arguments(L, kv8, kw):
    from qqq_amd import _lib

    assert _pre(L, kv8, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_prefill_attn_paged_kv8:" if kv8 else "qqq_prefill_attn_paged:")


@pytest.mark.parametrize("kv8", [False, True])
def test_workspace_holds_the_fp16_rows_where_o_fp16_is_null(L, kv8):
    from qqq_amd import _lib

    need = L.qqq_prefill_attn_workspace_bytes(40, 32, 128)
    assert need == 40 * 32 * 128 * 2
    assert L.qqq_prefill_attn_workspace_bytes(0, 32, 128) == 0 and L.qqq_prefill_attn_workspace_bytes(40, 32, 96) == 0
    assert L.qqq_prefill_attn_workspace_bytes(40, 256, 128) == 0  # h * d above 16384
    assert _pre(L, kv8, o=None, wsb=need - 1) == ERR_ARG and "workspace" in _lib.last_error()
    assert _lib.last_error().startswith("qqq_prefill_attn_paged")


def test_m0_and_b0_are_no_ops_with_null_pointers(L):
    z = None
    for m, b in ((0, 3), (5, 0), (0, 0)):
        assert L.qqq_prefill_attn_paged(z, z, z, z, 0, z, z, 1.0, z, z, z, z, 0, m, b, 32, 8, 128, 4, 16, 64, 0, z) == 0
        assert L.qqq_prefill_attn_paged_kv8(z, z, z, z, z, z, 0, z, z, 1.0, z, z, z, z, 0, m, b, 32, 8, 128, 4, 16, 64, 0, z) == 0
        for kv8 in (False, True):
            assert _pre(L, kv8, m=m, b=b) == 0


def test_prefill_kernels_in_the_code_object_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB) if k["demangled"].startswith("qqq_prefill_")}
    attn = {f"qqq_prefill_attn_kernel<{d},{kv8}>" for d in (64, 128) for kv8 in ("false", "true")}
    quant = {f"qqq_prefill_quant_kernel<{v},512>" for v in (1, 2, 4)}
    assert set(ks) == attn | quant
    for k in ks.values():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    for n in attn:
        d = 64 if "<64," in n else 128
        k = ks[n]
        assert k["max_flat_workgroup_size"] == 256 and k["vgpr_count"] + k["agpr_count"] <= 256, k  # two workgroups of four waves per CU
        # LDS: one 64-key tile of K (rows of 2d + 16 bytes) and of V (2d + 32 bytes), and the keys' scales of an int8 pool
        assert 64 * (4 * d + 48) <= k["group_segment_fixed_size"] <= 64 * (4 * d + 48) + 256, k
    for n in quant:
        assert ks[n]["max_flat_workgroup_size"] == 512 and ks[n]["group_segment_fixed_size"] <= 64, ks[n]
    # nothing of this feature joined the kernel families other tests pin
    assert not any("prefill" in k["demangled"] for k in code_object.kernels(build.LIB)
                   if k["demangled"].startswith(("qqq_paged_", "qqq_decode_", "qqq_kv8_")))


def _cpu_args(d=64, kv8=False):
    dt = torch.int8 if kv8 else torch.float16
    kp = torch.zeros((4, 2, 16, d), dtype=dt)
    sc = torch.zeros((4, 2, 16), dtype=torch.float32)
    return kp, kp.clone(), sc, sc.clone()


def test_cpu_tensors_raise():
    from qqq_amd import PagedKVCache, QuantLlamaAttention, ops, prefill_attention_paged, prefill_attention_paged_kv8

    assert prefill_attention_paged is ops.prefill_attention_paged and prefill_attention_paged_kv8 is ops.prefill_attention_paged_kv8
    d = 64
    q = torch.zeros((3, 4, d), dtype=torch.float16)
    cu = torch.tensor([0, 3], dtype=torch.int32)
    sp = torch.zeros(1, dtype=torch.int64)
    table = torch.zeros((1, 2), dtype=torch.int32)
    kp, vp, _, _ = _cpu_args(d)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.prefill_attention_paged(q, kp, vp, table, cu, sp, 0.125)
    kp, vp, ks, vs = _cpu_args(d, kv8=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.prefill_attention_paged_kv8(q, kp, vp, ks, vs, table, cu, sp, 0.125)
    attn = QuantLlamaAttention(256, 4, 2, -1).fuse_prefill()
    for dt in (torch.float16, torch.int8):
        cache = PagedKVCache(1, 4, 2, 64, 16, dtype=dt)
        cache.add(0)
        with pytest.raises(RuntimeError, match="no CPU path"):
            attn(torch.zeros((3, 256), dtype=torch.float16), cache, cache.step([0], [3]))


def test_fake_implementations_give_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from qqq_amd import ops

    h, kvh, d, nb, bs, m, b, w = 28, 4, 128, 12, 32, 9, 3, 5
    with FakeTensorMode():
        q = torch.empty((m, h, d), dtype=torch.float16)
        kp16 = torch.empty((nb, kvh, bs, d), dtype=torch.float16)
        kp8 = torch.empty((nb, kvh, bs, d), dtype=torch.int8)
        sc = torch.empty((nb, kvh, bs), dtype=torch.float32)
        table = torch.empty((b, w), dtype=torch.int32)
        cu = torch.empty((b + 1,), dtype=torch.int32)
        sp = torch.empty((b,), dtype=torch.int64)
        for fp16 in (False, True):
            outs = (torch.ops.qqq_amd.prefill_attn_paged(q, kp16, kp16, table, cu, sp, 0.1, None, fp16),
                    torch.ops.qqq_amd.prefill_attn_paged_kv8(q, kp8, kp8, sc, sc, table, cu, sp, 0.1, 100, fp16),
                    ops.prefill_attention_paged(q, kp16, kp16, table, cu, sp, 0.1, return_fp16=True),
                    ops.prefill_attention_paged_kv8(q, kp8, kp8, sc, sc, table, cu, sp, 0.1, max_len=100, return_fp16=True))
            for i, out in enumerate(outs):
                assert len(out) == 3
                assert out[0].shape == (m, h * d) and out[0].dtype == torch.int8
                assert out[1].shape == (m, 1) and out[1].dtype == torch.float32
                want = (m, h * d) if (fp16 or i >= 2) else (0,)
                assert out[2].shape == want and out[2].dtype == torch.float16
        assert len(ops.prefill_attention_paged(q, kp16, kp16, table, cu, sp, 0.1)) == 2
        with pytest.raises(RuntimeError, match="cu_tokens"):
            ops.prefill_attention_paged(q, kp16, kp16, table, sp, sp, 0.1)


def test_step_metadata_of_a_ragged_step_across_block_boundaries():
    from qqq_amd import PagedKVCache

    c = PagedKVCache(1, 12, 2, 64, 16)
    for sid in ("a", "b", "c"):
        c.add(sid)
    st = c.step(["a", "b", "c"], [5, 16, 35])
    assert st.cu_tokens.dtype == torch.int32 and st.start_pos.dtype == torch.int64
    assert st.cu_tokens.tolist() == [0, 5, 21, 56] and st.start_pos.tolist() == [0, 0, 0]
    st = c.step(["a", "b", "c"], [1, 1, 1])  # a decode step carries them too
    assert st.decode and st.cu_tokens.tolist() == [0, 1, 2, 3] and st.start_pos.tolist() == [5, 16, 35]
    st = c.step(["c", "a"], [30, 12])  # a chunk that crosses two block boundaries, another order
    assert st.cu_tokens.tolist() == [0, 30, 42] and st.start_pos.tolist() == st.starts == [36, 6]
    assert st.pos.tolist() == list(range(36, 66)) + list(range(6, 18)) and st.last_pos.tolist() == [65, 17]  # the old fields are unchanged
    assert st.block_table.tolist() == [[2, 3, 4, 6, 7], [0, 8, 0, 0, 0]] and st.max_len == 66 and not st.decode
    for i in range(2):  # token t of sequence i sits at start_pos[i] + t - cu_tokens[i]
        lo, hi = st.cu_tokens[i].item(), st.cu_tokens[i + 1].item()
        assert st.pos[lo:hi].tolist() == [st.start_pos[i].item() + t - lo for t in range(lo, hi)]


def test_fuse_prefill_is_a_flag_outside_the_state_dict():
    from qqq_amd import QuantLlamaAttention, QuantLlamaDecoderLayer

    attn = QuantLlamaAttention(256, 4, 2, -1)
    keys = sorted(attn.state_dict())
    assert not attn.prefill_fused
    assert attn.fuse_prefill() is attn and attn.prefill_fused and not attn.decode_fused
    assert sorted(attn.state_dict()) == keys
    attn.load_state_dict(attn.state_dict())
    assert attn.prefill_fused  # kept, like fuse_decode()
    assert attn.unfuse_prefill() is attn and not attn.prefill_fused
    layer = QuantLlamaDecoderLayer(256, 4, 2, 512, -1)
    keys = sorted(layer.state_dict())
    assert not layer.prefill_fused
    assert layer.fuse_prefill() is layer and layer.prefill_fused and layer.self_attn.prefill_fused and not layer.decode_fused
    assert sorted(layer.state_dict()) == keys
    assert layer.unfuse_prefill() is layer and not layer.self_attn.prefill_fused
