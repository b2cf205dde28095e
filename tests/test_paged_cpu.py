"""The paged KV cache without a GPU: the C-ABI of include/qqq_amd_paged.h (declared set, exports, argument checks before any launch), the
qqq_paged_* kernels' resources in the gfx950 code object, the ops' CPU refusal and fake implementations, and PagedKVCache on CPU tensors:
allocation order, step() metadata, exhaustion, free and reuse, gather / dequant, nbytes."""
import os
import sys

import pytest
import torch

import kv8_ref as K8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 17
ENTRIES = {"qqq_rope_qkv_paged", "qqq_rope_qkv_paged_kv8", "qqq_decode_attn_paged", "qqq_decode_attn_paged_kv8"}


@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def test_header_declares_the_four_functions_and_the_library_exports_them(L):
    from qqq_amd import _abi

    names = set(_abi.prototypes(os.path.join(ROOT, "include", "qqq_amd_paged.h")))
    assert names == ENTRIES
    for n in names:
        assert hasattr(L, n), n
    assert L.qqq_amd_abi_version() == 4


# fake device addresses with the alignment the entry points ask for: the calls below must fail in the checks, before any launch
A16, A8, A4 = 0x10000, 0x20008, 0x30004
WS = 1 << 30


def _rope(L, kv8, q=A16, ld_q=None, k=A16, ld_k=None, v=A16, ld_v=None, cos=A16, sin=A16, table_len=4096, pos=A8, slots=A8, q_out=A16,
          kp=A16, vp=A16, ks=A4, vs=A4, m=6, h=32, kvh=8, d=128, nb=64, bs=128):
    ld_q = h * d if ld_q is None else ld_q
    ld_k = kvh * d if ld_k is None else ld_k
    ld_v = kvh * d if ld_v is None else ld_v
    head = (q, ld_q, k, ld_k, v, ld_v, cos, sin, table_len, pos, slots, q_out, kp, vp)
    tail = (m, h, kvh, d, nb, bs, 0, None)
    return L.qqq_rope_qkv_paged_kv8(*head, ks, vs, *tail) if kv8 else L.qqq_rope_qkv_paged(*head, *tail)


ROPE_BAD = [dict(kp=None), dict(vp=None), dict(q=None), dict(k=None), dict(v=None), dict(cos=None), dict(sin=None), dict(pos=None),
            dict(slots=None), dict(q_out=None), dict(d=96), dict(d=32), dict(d=256), dict(d=16), dict(h=30), dict(kvh=0), dict(h=0),
            dict(kp=A16 + 8), dict(vp=A16 + 4), dict(q=A16 + 8), dict(pos=A8 + 4), dict(slots=A8 + 4), dict(q_out=A16 + 2), dict(ld_q=4095),
            dict(ld_k=1028), dict(ld_v=1020), dict(m=-1), dict(nb=-1), dict(nb=0), dict(table_len=-1), dict(bs=8), dict(bs=24), dict(bs=512),
            dict(bs=0), dict(bs=-16), dict(nb=1 << 24, bs=256)]
ROPE_BAD_KV8 = [dict(ks=None), dict(vs=None), dict(ks=A4 + 2), dict(vs=A4 + 1)]


@pytest.mark.parametrize("kv8,kw", [(False, kw) for kw in ROPE_BAD] + [(True, kw) for kw in ROPE_BAD + ROPE_BAD_KV8])
def test_rope_qkv_paged_rejects_bad_arguments(L, kv8, kw):
    from qqq_amd import _lib

    assert _rope(L, kv8, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_rope_qkv_paged_kv8:" if kv8 else "qqq_rope_qkv_paged:")


def _dec(L, kv8, q=A16, kp=A16, vp=A16, ks=A4, vs=A4, table=A4, stride=32, pos=A8, scale=0.088, o=A16, xq=A8, s1=A4, ws=A16, wsb=WS, b=2,
         h=32, kvh=8, d=128, nb=64, bs=128, max_len=4096):
    tail = (table, stride, pos, scale, o, xq, s1, ws, wsb, b, h, kvh, d, nb, bs, max_len, 0, None)
    return L.qqq_decode_attn_paged_kv8(q, kp, vp, ks, vs, *tail) if kv8 else L.qqq_decode_attn_paged(q, kp, vp, *tail)


DEC_BAD = [dict(q=None), dict(kp=None), dict(vp=None), dict(table=None), dict(pos=None), dict(ws=None), dict(o=None, xq=None, s1=None),
           dict(xq=None), dict(s1=None), dict(d=96), dict(d=256), dict(d=32), dict(h=72), dict(h=30), dict(h=0), dict(kvh=0),
           dict(h=256, kvh=32), dict(q=A16 + 8), dict(kp=A16 + 2), dict(vp=A16 + 4), dict(table=A4 + 2), dict(table=A4 + 1), dict(pos=A8 + 4),
           dict(o=A16 + 8), dict(xq=A8 + 4), dict(s1=A4 + 2), dict(ws=A16 + 8), dict(wsb=0), dict(wsb=1000), dict(max_len=0),
           dict(max_len=-1), dict(max_len=4097), dict(stride=31), dict(stride=0, max_len=1), dict(stride=-1), dict(b=-1), dict(b=65536),
           dict(bs=8, stride=512), dict(bs=24, stride=512), dict(bs=512, stride=512), dict(nb=0), dict(nb=-1), dict(nb=1 << 24, bs=256)]
DEC_BAD_KV8 = [dict(ks=None), dict(vs=None), dict(ks=A4 + 2), dict(vs=A4 + 1)]


@pytest.mark.parametrize("kv8,kw", [(False, kw) for kw in DEC_BAD] + [(True, kw) for kw in DEC_BAD + DEC_BAD_KV8])
def test_decode_attn_paged_rejects_bad_arguments(L, kv8, kw):
    from qqq_amd import _lib

    assert _dec(L, kv8, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_decode_attn_paged_kv8:" if kv8 else "qqq_decode_attn_paged:")


@pytest.mark.parametrize("kv8", [False, True])
def test_workspace_check_uses_the_contiguous_kernels_workspace_size(L, kv8):
    from qqq_amd import _lib

    need = L.qqq_decode_attn_workspace_bytes(2, 32, 8, 128, 4096)
    assert need > 0
    assert _dec(L, kv8, wsb=need - 1) == ERR_ARG and "workspace" in _lib.last_error()
    # max_len bounds the workspace, not the table: a short max_len under a wide table needs less
    small = L.qqq_decode_attn_workspace_bytes(2, 32, 8, 128, 100)
    assert small < need and _dec(L, kv8, max_len=100, wsb=small - 1) == ERR_ARG and "workspace" in _lib.last_error()


def test_m0_and_b0_are_no_ops_with_null_pointers(L):
    for kv8 in (False, True):
        assert _dec(L, kv8, b=0) == 0 and _rope(L, kv8, m=0) == 0
    z = None
    assert L.qqq_rope_qkv_paged(z, 0, z, 0, z, 0, z, z, 0, z, z, z, z, z, 0, 32, 8, 128, 4, 16, 0, z) == 0
    assert L.qqq_rope_qkv_paged_kv8(z, 0, z, 0, z, 0, z, z, 0, z, z, z, z, z, z, z, 0, 32, 8, 128, 4, 16, 0, z) == 0
    assert L.qqq_decode_attn_paged(z, z, z, z, 0, z, 1.0, z, z, z, z, 0, 0, 32, 8, 128, 4, 16, 64, 0, z) == 0
    assert L.qqq_decode_attn_paged_kv8(z, z, z, z, z, z, 0, z, 1.0, z, z, z, z, 0, 0, 32, 8, 128, 4, 16, 64, 0, z) == 0


def test_paged_kernels_in_the_code_object_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB) if k["demangled"].startswith("qqq_paged_")}
    assert set(ks) == {"qqq_paged_rope_qkv_kernel<128>", "qqq_paged_kv8_rope_qkv_kernel<128>", "qqq_paged_decode_split_kernel<64>",
                       "qqq_paged_decode_split_kernel<128>", "qqq_paged_kv8_decode_split_kernel<64>",
                       "qqq_paged_kv8_decode_split_kernel<128>"}
    for k in ks.values():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    for n in ("qqq_paged_rope_qkv_kernel<128>", "qqq_paged_kv8_rope_qkv_kernel<128>"):
        assert ks[n]["group_segment_fixed_size"] == 0 and ks[n]["max_flat_workgroup_size"] == 128, ks[n]  # no LDS in the write kernels
    for fam in ("qqq_paged_decode_split_kernel", "qqq_paged_kv8_decode_split_kernel"):
        for d in (64, 128):
            k = ks[f"{fam}<{d}>"]
            assert k["max_flat_workgroup_size"] == 256 and k["vgpr_count"] + k["agpr_count"] <= 128, k  # four waves per SIMD
            assert k["group_segment_fixed_size"] <= 4 * 8 * d * 4 + 256, k  # LDS: the contiguous kernels' bound (the four waves' partials)


def _cpu_args(d=64, kv8=False):
    dt = torch.int8 if kv8 else torch.float16
    kp = torch.zeros((4, 2, 16, d), dtype=dt)
    sc = torch.zeros((4, 2, 16), dtype=torch.float32)
    return kp, kp.clone(), sc, sc.clone()


def test_cpu_tensors_raise():
    from qqq_amd import PagedKVCache, QuantLlamaAttention, ops

    d = 64
    q = torch.zeros((1, 4, 1, d), dtype=torch.float16)
    pos = torch.zeros(1, dtype=torch.int64)
    table = torch.zeros((1, 2), dtype=torch.int32)
    rows = torch.zeros((1, 4 * d), dtype=torch.float16)
    kv = torch.zeros((1, 2 * d), dtype=torch.float16)
    tab = torch.zeros((16, d), dtype=torch.float16)
    kp, vp, _, _ = _cpu_args(d)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.decode_attention_paged(q, kp, vp, table, pos, 0.125)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rope_qkv_paged(rows, kv, kv.clone(), tab, tab.clone(), pos, pos.clone(), kp, vp)
    kp, vp, ks, vs = _cpu_args(d, kv8=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.decode_attention_paged_kv8(q, kp, vp, ks, vs, table, pos, 0.125)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rope_qkv_paged_kv8(rows, kv, kv.clone(), tab, tab.clone(), pos, pos.clone(), kp, vp, ks, vs)
    attn = QuantLlamaAttention(256, 4, 2, -1)
    for dt in (torch.float16, torch.int8):
        cache = PagedKVCache(1, 4, 2, 64, 16, dtype=dt)
        cache.add(0)
        with pytest.raises(RuntimeError, match="no CPU path"):
            attn(torch.zeros((1, 256), dtype=torch.float16), cache, cache.step([0], [1]))


def test_paged_cache_refuses_head_shapes_the_decode_kernel_does_not_take_and_a_plain_start():
    from qqq_amd import PagedKVCache, QuantLlamaAttention

    xq, s1 = torch.zeros((1, 256), dtype=torch.int8), torch.zeros((1, 1), dtype=torch.float32)
    cache = PagedKVCache(1, 4, 2, 32, 16)
    cache.add("a")
    with pytest.raises(NotImplementedError, match="paged KV cache"):
        QuantLlamaAttention(256, 8, 2, -1).forward_int8(xq, s1, cache, cache.step(["a"], [1]))  # head_dim 32
    with pytest.raises(RuntimeError, match="PagedStep"):
        QuantLlamaAttention(256, 4, 2, -1).forward_int8(xq, s1, PagedKVCache(1, 4, 2, 64, 16), 0)


def test_fake_implementations_give_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from qqq_amd import ops

    h, kvh, d, nb, bs, m, b, w = 28, 4, 128, 12, 32, 9, 3, 5
    with FakeTensorMode():
        q = torch.empty((m, h * d), dtype=torch.float16)
        k = torch.empty((m, kvh * d), dtype=torch.float16)
        tab = torch.empty((100, d), dtype=torch.float16)
        pos = torch.empty((m,), dtype=torch.int64)
        kp16 = torch.empty((nb, kvh, bs, d), dtype=torch.float16)
        kp8 = torch.empty((nb, kvh, bs, d), dtype=torch.int8)
        sc = torch.empty((nb, kvh, bs), dtype=torch.float32)
        table = torch.empty((b, w), dtype=torch.int32)
        bpos = torch.empty((b,), dtype=torch.int64)
        vp16, vp8, vsc = torch.empty_like(kp16), torch.empty_like(kp8), torch.empty_like(sc)
        for out in (ops.rope_qkv_paged(q, k, k, tab, tab, pos, pos, kp16, vp16),
                    ops.rope_qkv_paged_kv8(q, k, k, tab, tab, pos, pos, kp8, vp8, sc, vsc)):
            assert out.shape == (m, h, d) and out.dtype == torch.float16
        for qd in (torch.empty((b, h, d), dtype=torch.float16), torch.empty((b, h, 1, d), dtype=torch.float16)):
            for fp16 in (False, True):
                outs = (ops.decode_attention_paged(qd, kp16, kp16, table, bpos, 0.1, return_fp16=fp16),
                        ops.decode_attention_paged_kv8(qd, kp8, kp8, sc, sc, table, bpos, 0.1, max_len=100, return_fp16=fp16))
                for out in outs:
                    assert len(out) == (3 if fp16 else 2)
                    assert out[0].shape == (b, h * d) and out[0].dtype == torch.int8
                    assert out[1].shape == (b, 1) and out[1].dtype == torch.float32
                    if fp16:
                        assert out[2].shape == (b, h * d) and out[2].dtype == torch.float16


# ---- PagedKVCache on CPU tensors

def test_layout_and_nbytes():
    from qqq_amd import PagedKVCache

    L_, nb, kvh, d, bs = 3, 10, 4, 128, 32
    c = PagedKVCache(L_, nb, kvh, d, bs)
    assert c.dtype == torch.float16 and not c.quantized and not hasattr(c, "k_scale") and c.free_blocks == nb
    assert len(c.k) == len(c.v) == L_
    assert all(t.dtype == torch.float16 and t.shape == (nb, kvh, bs, d) and t.is_contiguous() and not t.any() for t in c.k + c.v)
    assert c.nbytes == 4 * L_ * nb * kvh * bs * d == sum(t.numel() * t.element_size() for t in c.k + c.v)
    c8 = PagedKVCache(L_, nb, kvh, d, bs, dtype=torch.int8)
    assert c8.quantized and len(c8.k_scale) == len(c8.v_scale) == L_
    assert all(t.dtype == torch.int8 and t.shape == (nb, kvh, bs, d) for t in c8.k + c8.v)
    assert all(t.dtype == torch.float32 and t.shape == (nb, kvh, bs) and t.is_contiguous() for t in c8.k_scale + c8.v_scale)
    assert c8.nbytes == 2 * L_ * nb * kvh * bs * (d + 4) == sum(t.numel() * t.element_size() for t in c8.k + c8.v + c8.k_scale + c8.v_scale)
    for dt in (torch.bfloat16, torch.float32, torch.uint8):
        with pytest.raises(ValueError, match="dtype"):
            PagedKVCache(1, 1, 1, 64, 16, dtype=dt)
    for bad in (8, 24, 512, 0):
        with pytest.raises(ValueError, match="block_size"):
            PagedKVCache(1, 4, 1, 64, bad)


def test_allocation_order_and_step_metadata_across_block_boundaries():
    from qqq_amd import PagedKVCache, PagedStep

    bs = 16
    c = PagedKVCache(1, 12, 2, 64, bs)
    for sid in ("a", "b", "c"):
        c.add(sid)
    assert c.free_blocks == 12 and c.length("a") == 0 and c.blocks("a") == []  # a sequence owns nothing before its first step
    st = c.step(["a", "b", "c"], [5, 16, 35])  # ragged prefill: 1, 1 and 3 blocks, handed out in order 0, 1, 2 ...
    assert isinstance(st, PagedStep) and not st.decode
    assert (c.blocks("a"), c.blocks("b"), c.blocks("c")) == ([0], [1], [2, 3, 4]) and c.free_blocks == 7
    assert (st.seq_ids, st.counts, st.starts, st.max_len) == (["a", "b", "c"], [5, 16, 35], [0, 0, 0], 35)
    assert st.pos.dtype == torch.int64 and st.slots.dtype == torch.int64 and st.block_table.dtype == torch.int32
    assert st.last_pos.dtype == torch.int64
    assert st.pos.tolist() == list(range(5)) + list(range(16)) + list(range(35))
    want = list(range(5)) + [16 + i for i in range(16)] + [32 + i for i in range(35)]  # blocks 2, 3, 4 are adjacent: slots run on
    assert st.slots.tolist() == want
    assert st.block_table.tolist() == [[0, 0, 0], [1, 0, 0], [2, 3, 4]] and st.last_pos.tolist() == [4, 15, 34]
    # a decode step: b is exactly at a block boundary and takes a new block, the others stay inside theirs
    st = c.step(["a", "b", "c"], [1, 1, 1])
    assert st.decode and st.starts == [5, 16, 35] and st.max_len == 36
    assert c.blocks("b") == [1, 5] and c.free_blocks == 6
    assert st.pos.tolist() == [5, 16, 35] and st.slots.tolist() == [5, 5 * bs, 4 * bs + 3]
    assert st.block_table.tolist() == [[0, 0, 0], [1, 5, 0], [2, 3, 4]] and st.last_pos.tolist() == [5, 16, 35]
    # a chunk that crosses two boundaries, for a subset of the sequences in another order
    st = c.step(["c", "a"], [30, 12])
    assert not st.decode and st.starts == [36, 6] and st.max_len == 66
    assert c.blocks("c") == [2, 3, 4, 6, 7] and c.blocks("a") == [0, 8] and (c.length("c"), c.length("a")) == (66, 18)
    blocks_c = [2, 3, 4, 6, 7]
    assert st.slots.tolist() == [blocks_c[p // bs] * bs + p % bs for p in range(36, 66)] + [6 + i for i in range(10)] + [8 * bs, 8 * bs + 1]
    assert st.block_table.tolist() == [[2, 3, 4, 6, 7], [0, 8, 0, 0, 0]] and st.last_pos.tolist() == [65, 17]
    for bad in (dict(seq_ids=["a", "a"], counts=[1, 1]), dict(seq_ids=["a"], counts=[0]), dict(seq_ids=[], counts=[]),
                dict(seq_ids=["a"], counts=[1, 2])):
        with pytest.raises(ValueError):
            c.step(**bad)
    with pytest.raises(KeyError):
        c.step(["nobody"], [1])
    with pytest.raises(KeyError):
        c.add("a")


def test_exhaustion_raises_and_changes_nothing_then_free_and_reuse():
    from qqq_amd import PagedKVCache

    c = PagedKVCache(1, 6, 1, 64, 16)
    c.add(1)
    c.add(2)
    c.step([1, 2], [40, 20])  # 3 + 2 blocks
    assert c.blocks(1) == [0, 1, 2] and c.blocks(2) == [3, 4] and c.free_blocks == 1
    before = (c.blocks(1), c.blocks(2), c.length(1), c.length(2), c.free_blocks)
    with pytest.raises(RuntimeError, match="exhausted"):
        c.step([1, 2], [9, 13])  # sequence 1 needs one more block (49 keys), sequence 2 one more (33 keys): two, one is free
    assert (c.blocks(1), c.blocks(2), c.length(1), c.length(2), c.free_blocks) == before
    st = c.step([1], [9])  # ... and one of them alone fits
    assert c.blocks(1) == [0, 1, 2, 5] and c.free_blocks == 0 and st.last_pos.tolist() == [48]
    c.free(2)
    assert c.free_blocks == 2
    with pytest.raises(KeyError):
        c.length(2)
    with pytest.raises(KeyError):
        c.free(2)
    c.add(3)
    st = c.step([3], [20])
    assert sorted(c.blocks(3)) == [3, 4] and c.free_blocks == 0  # the freed blocks, nothing else
    assert st.slots.tolist() == [c.blocks(3)[p // 16] * 16 + p % 16 for p in range(20)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_gather_values(dtype):
    from qqq_amd import PagedKVCache

    nb, kvh, d, bs = 7, 3, 64, 16
    c = PagedKVCache(2, nb, kvh, d, bs, dtype=dtype)
    c.add("x")
    c.step(["x"], [3])   # block 0
    c.add("y")
    c.step(["y"], [40])  # blocks 1, 2, 3
    c.step(["x"], [20])  # block 4: x's blocks are 0, 4 -- not adjacent
    assert c.blocks("x") == [0, 4] and c.blocks("y") == [1, 2, 3]
    g = torch.Generator().manual_seed(3)
    src = {}
    for name, pools, scales in (("k", c.k, getattr(c, "k_scale", None)), ("v", c.v, getattr(c, "v_scale", None))):
        x = (torch.randn((nb, kvh, bs, d), generator=g) * torch.rand((nb, kvh, bs, 1), generator=g) * 8).half()
        if dtype == torch.int8:
            pools[1], scales[1] = K8.quant_rows(x)
            src[name] = K8.dequant64(pools[1], scales[1]).half()  # fp16(float(code) * scale): the fp32 product is exact
        else:
            pools[1] = x
            src[name] = x
    for sid, n in (("x", None), ("x", 17), ("x", 16), ("x", 1), ("y", None), ("y", 33), ("y", 0)):
        k, v = c.gather(1, sid, n)
        n = c.length(sid) if n is None else n
        for got, name in ((k, "k"), (v, "v")):
            assert got.dtype == torch.float16 and got.shape == (1, kvh, n, d) and got.is_contiguous()
            for p in range(n):
                blk = c.blocks(sid)[p // bs]
                assert torch.equal(got[0, :, p], src[name][blk, :, p % bs]), (sid, n, p)
    with pytest.raises(ValueError):
        c.gather(1, "x", 24)


def test_kvcache_is_unchanged():
    from qqq_amd import KVCache

    c = KVCache(2, 3, 4, 64, 20)
    assert c.dtype == torch.float16 and not c.quantized and not hasattr(c, "k_scale")
    assert all(t.dtype == torch.float16 and t.shape == (3, 4, 20, 64) for t in c.k + c.v) and c.nbytes == 4 * 2 * 3 * 4 * 20 * 64
    assert torch.equal(c.positions(7, 1), torch.tensor([7, 7, 7])) and torch.equal(c.positions(2, 2), torch.tensor([2, 3, 2, 3, 2, 3]))
    c8 = KVCache(1, 2, 2, 64, 8, dtype=torch.int8)
    assert c8.quantized and c8.k_scale[0].shape == (2, 2, 8) and c8.nbytes == 2 * 2 * 2 * 8 * 68
