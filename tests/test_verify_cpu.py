"""The verify chunk's attention without a GPU (include/qqq_amd_verify.h): the header and the exports, the argument checks of the two entry
points with fake aligned addresses, the workspace size, the kernels' entries in the gfx950 code object, the ops' CPU refusal and fake
shapes, the routing of fuse_verify() with host stubs for the ops, and what SpecDecodeLoop's constructor accepts."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 17
ENTRIES = {"qqq_verify_attn_paged", "qqq_verify_attn_paged_kv8", "qqq_verify_attn_workspace_bytes"}


@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def test_header_declares_the_three_functions_and_the_library_exports_them(L):
    from qqq_amd import _abi

    names = set(_abi.prototypes(os.path.join(ROOT, "include", "qqq_amd_verify.h")))
    assert names == ENTRIES
    for n in names:
        assert hasattr(L, n), n
    assert L.qqq_amd_abi_version() == 4  # (a change of the header rebuilds the library: tests/test_abi_cpu.py)


# fake device addresses with the alignment the entry points ask for: the calls below must fail in the checks, before any launch
A16, A8, A4 = 0x10000, 0x20008, 0x30004
WS = 1 << 30


def _ver(L, kv8, q=A16, kp=A16, vp=A16, ks=A4, vs=A4, table=A4, stride=32, start=A8, scale=0.088, o=A16, xq=A8, s1=A4, ws=A16, wsb=WS, b=2,
         t=5, h=32, kvh=8, d=128, nb=64, bs=128, max_len=4096):
    tail = (table, stride, start, scale, o, xq, s1, ws, wsb, b, t, h, kvh, d, nb, bs, max_len, 0, None)
    return L.qqq_verify_attn_paged_kv8(q, kp, vp, ks, vs, *tail) if kv8 else L.qqq_verify_attn_paged(q, kp, vp, *tail)


# DEC_BAD of tests/test_paged_cpu.py with `start` for `pos`, and the chunk's own limits
VER_BAD = [dict(q=None), dict(kp=None), dict(vp=None), dict(table=None), dict(start=None), dict(ws=None), dict(o=None, xq=None, s1=None),
           dict(xq=None), dict(s1=None), dict(d=96), dict(d=256), dict(d=32), dict(h=72), dict(h=30), dict(h=0), dict(kvh=0),
           dict(h=256, kvh=32), dict(q=A16 + 8), dict(kp=A16 + 2), dict(vp=A16 + 4), dict(table=A4 + 2), dict(table=A4 + 1),
           dict(start=A8 + 4), dict(o=A16 + 8), dict(xq=A8 + 4), dict(s1=A4 + 2), dict(ws=A16 + 8), dict(wsb=0), dict(wsb=1000),
           dict(max_len=0), dict(max_len=-1), dict(max_len=4097), dict(stride=31), dict(stride=0, max_len=1), dict(stride=-1), dict(b=-1),
           dict(b=65536, t=1), dict(bs=8, stride=512), dict(bs=24, stride=512), dict(bs=512, stride=512), dict(nb=0), dict(nb=-1),
           dict(nb=1 << 24, bs=256),
           dict(t=0), dict(t=17), dict(t=-1), dict(h=64, kvh=8, t=9), dict(b=4096, t=16), dict(b=13108, t=5)]
VER_BAD_KV8 = [dict(ks=None), dict(vs=None), dict(ks=A4 + 2), dict(vs=A4 + 1)]


@pytest.mark.parametrize("kv8,kw", [(False, kw) for kw in VER_BAD] + [(True, kw) for kw in VER_BAD + VER_BAD_KV8])
def test_verify_attn_paged_rejects_bad_arguments(L, kv8, kw):
    from qqq_amd import _lib

    assert _ver(L, kv8, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_verify_attn_paged_kv8:" if kv8 else "qqq_verify_attn_paged:")


def test_the_refused_chunk_shapes_are_the_ones_meant():
    assert (64 // 8) * 9 == 72 and 4096 * 16 == 65536 and 13108 * 5 > 65535 >= 13107 * 5


@pytest.mark.parametrize("kv8", [False, True])
def test_workspace_is_the_decode_workspace_of_every_token(L, kv8):
    from qqq_amd import _lib

    for b, t, h, kvh, d, max_len in ((2, 5, 32, 8, 128, 4096), (1, 16, 4, 4, 64, 640), (16, 3, 32, 32, 128, 100), (4095, 16, 8, 2, 64, 17)):
        need = L.qqq_verify_attn_workspace_bytes(b, t, h, kvh, d, max_len)
        assert need > 0 and need == L.qqq_decode_attn_workspace_bytes(b * t, h, kvh, d, max_len)
    assert L.qqq_verify_attn_workspace_bytes(0, 5, 32, 8, 128, 4096) == 0
    for bad in ((2, 0), (2, 17), (4096, 16)):
        assert L.qqq_verify_attn_workspace_bytes(*bad, 32, 8, 128, 4096) == 0
    need = L.qqq_verify_attn_workspace_bytes(2, 5, 32, 8, 128, 4096)
    assert _ver(L, kv8, wsb=need - 1) == ERR_ARG and "workspace" in _lib.last_error()
    # a decode call's workspace is too short for a chunk
    assert _ver(L, kv8, wsb=L.qqq_decode_attn_workspace_bytes(2, 32, 8, 128, 4096)) == ERR_ARG and "workspace" in _lib.last_error()


def test_b0_is_a_no_op_with_null_pointers(L):
    for kv8 in (False, True):
        assert _ver(L, kv8, b=0) == 0
    z = None
    assert L.qqq_verify_attn_paged(z, z, z, z, 0, z, 1.0, z, z, z, z, 0, 0, 5, 32, 8, 128, 4, 16, 64, 0, z) == 0
    assert L.qqq_verify_attn_paged_kv8(z, z, z, z, z, z, 0, z, 1.0, z, z, z, z, 0, 0, 5, 32, 8, 128, 4, 16, 64, 0, z) == 0


def test_verify_kernels_in_the_code_object_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB) if k["demangled"].startswith("qqq_verify_")}
    split = {f"qqq_verify_{fam}split_kernel<{d},{nq}>" for fam in ("", "kv8_") for d in (64, 128) for nq in (1, 2, 4)}
    combine = {f"qqq_verify_combine_kernel<{v},512>" for v in (1, 2, 4)}
    assert len(split) == 12 and set(ks) == split | combine
    for k in ks.values():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    for n in split:
        d, nq = (int(x) for x in n[n.index("<") + 1:-1].split(","))
        k = ks[n]
        assert k["max_flat_workgroup_size"] == 256, k
        # LDS: one 16-row tile of the four waves' partials per merge pass (Q^T waits in it), and the rows' (m, l)
        assert k["group_segment_fixed_size"] <= 4 * 16 * d * 4 + 2 * 4 * 16 * nq * 4 + 256, k
        regs = k["vgpr_count"]  # of the unified file: the accumulation registers (agpr_count) are part of it
        assert k["agpr_count"] == 0 or (nq, d) == (4, 128), k
        assert regs <= (128 if nq == 1 and not ("kv8" in n and d == 128) else 168 if nq == 1 else 256 if nq == 2 or d == 64 else 512), k
    for n in combine:  # the decode combine's row, inlined: its registers and LDS
        dec = {k["demangled"]: k for k in code_object.kernels(build.LIB)}[n.replace("verify", "decode")]
        assert ks[n]["max_flat_workgroup_size"] == 512 and ks[n]["group_segment_fixed_size"] == dec["group_segment_fixed_size"]
        assert ks[n]["vgpr_count"] <= dec["vgpr_count"] + 4, (ks[n], dec)


def _cpu_args(d=64, kv8=False):
    dt = torch.int8 if kv8 else torch.float16
    kp = torch.zeros((4, 2, 16, d), dtype=dt)
    sc = torch.zeros((4, 2, 16), dtype=torch.float32)
    return kp, kp.clone(), sc, sc.clone()


def test_cpu_tensors_raise():
    from qqq_amd import PagedKVCache, QuantLlamaAttention, ops, verify_attention_paged, verify_attention_paged_kv8

    assert verify_attention_paged is ops.verify_attention_paged and verify_attention_paged_kv8 is ops.verify_attention_paged_kv8
    d = 64
    q = torch.zeros((3, 4, d), dtype=torch.float16)
    start = torch.zeros(1, dtype=torch.int64)
    table = torch.zeros((1, 2), dtype=torch.int32)
    kp, vp, _, _ = _cpu_args(d)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.verify_attention_paged(q, kp, vp, table, start, 3, 0.125)
    kp, vp, ks, vs = _cpu_args(d, kv8=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.verify_attention_paged_kv8(q, kp, vp, ks, vs, table, start, 3, 0.125)
    attn = QuantLlamaAttention(256, 4, 2, -1).fuse_verify()
    for dt in (torch.float16, torch.int8):
        cache = PagedKVCache(1, 4, 2, 64, 16, dtype=dt)
        cache.add(0)
        with pytest.raises(RuntimeError, match="no CPU path"):
            attn(torch.zeros((3, 256), dtype=torch.float16), cache, cache.step([0], [3]))


def test_fake_implementations_give_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from qqq_amd import ops

    h, kvh, d, nb, bs, b, t, w = 28, 4, 128, 12, 32, 3, 5, 5
    m = b * t
    with FakeTensorMode():
        q = torch.empty((m, h, d), dtype=torch.float16)
        kp16 = torch.empty((nb, kvh, bs, d), dtype=torch.float16)
        kp8 = torch.empty((nb, kvh, bs, d), dtype=torch.int8)
        sc = torch.empty((nb, kvh, bs), dtype=torch.float32)
        table = torch.empty((b, w), dtype=torch.int32)
        start = torch.empty((b,), dtype=torch.int64)
        for fp16 in (False, True):
            outs = (torch.ops.qqq_amd.verify_attn_paged(q, kp16, kp16, table, start, t, 0.1, None, fp16),
                    torch.ops.qqq_amd.verify_attn_paged_kv8(q, kp8, kp8, sc, sc, table, start, t, 0.1, 100, fp16),
                    ops.verify_attention_paged(q, kp16, kp16, table, start, t, 0.1, return_fp16=True),
                    ops.verify_attention_paged_kv8(q, kp8, kp8, sc, sc, table, start, t, 0.1, max_len=100, return_fp16=True))
            for i, out in enumerate(outs):
                assert len(out) == 3
                assert out[0].shape == (m, h * d) and out[0].dtype == torch.int8
                assert out[1].shape == (m, 1) and out[1].dtype == torch.float32
                want = (m, h * d) if (fp16 or i >= 2) else (0,)
                assert out[2].shape == want and out[2].dtype == torch.float16
        assert len(ops.verify_attention_paged(q, kp16, kp16, table, start, t, 0.1)) == 2
        with pytest.raises(RuntimeError, match="q_out"):
            ops.verify_attention_paged(q, kp16, kp16, table, start, 4, 0.1)  # 15 rows are not 3 rows of 4 tokens
        with pytest.raises(RuntimeError, match="tokens"):
            ops.verify_attention_paged(q, kp16, kp16, table, start, 0, 0.1)


def test_fuse_verify_is_a_flag_outside_the_state_dict():
    from qqq_amd import QuantLlamaAttention, QuantLlamaDecoderLayer
    from test_step_cpu import _tiny_lm

    attn = QuantLlamaAttention(256, 4, 2, -1)
    keys = sorted(attn.state_dict())
    assert not attn.verify_fused
    assert attn.fuse_verify() is attn and attn.verify_fused and not attn.prefill_fused and not attn.decode_fused
    assert sorted(attn.state_dict()) == keys
    attn.load_state_dict(attn.state_dict())
    assert attn.verify_fused  # kept, like fuse_prefill()
    assert attn.unfuse_verify() is attn and not attn.verify_fused
    layer = QuantLlamaDecoderLayer(256, 4, 2, 512, -1)
    assert not layer.verify_fused
    assert layer.fuse_verify() is layer and layer.verify_fused and layer.self_attn.verify_fused and not layer.prefill_fused
    assert layer.unfuse_verify() is layer and not layer.self_attn.verify_fused
    lm = _tiny_lm()
    assert not any(layer.verify_fused for layer in lm.model.layers)
    assert lm.fuse_verify() is lm and all(layer.verify_fused for layer in lm.model.layers)
    assert lm.unfuse_verify() is lm and not any(layer.verify_fused for layer in lm.model.layers)
    assert lm.model.fuse_verify() is lm.model and all(layer.verify_fused for layer in lm.model.layers)
    assert lm.model.unfuse_verify() is lm.model and not any(layer.verify_fused for layer in lm.model.layers)


class _Routes:
    """host stubs for the ops _forward_paged may call: every call is recorded by name, outputs are zeros of the right shape"""

    def __init__(self, attn, monkeypatch):
        self.calls = []
        h, d = attn.num_heads, attn.head_dim

        def rope(q, k, v, cos, sin, pos, slots, *pools):
            return torch.zeros((q.shape[0], h, d), dtype=torch.float16)

        def quantised(name):
            def op(q_out, *rest, **kw):
                self.calls.append((name, kw.get("max_len")) + ((rest[-2],) if name.startswith("verify") else ()))
                rows = q_out.shape[0]
                return torch.zeros((rows, h * d), dtype=torch.int8), torch.zeros((rows, 1), dtype=torch.float32)
            return op

        for name in ("rope_qkv_paged", "rope_qkv_paged_kv8"):
            monkeypatch.setattr(f"qqq_amd.attention.ops.{name}", rope)
        for name in ("verify_attention_paged", "verify_attention_paged_kv8", "prefill_attention_paged", "prefill_attention_paged_kv8",
                     "decode_attention_paged", "decode_attention_paged_kv8"):
            monkeypatch.setattr(f"qqq_amd.attention.ops.{name}", quantised(name))

        def dynamic_quant(x):
            self.calls.append(("sdpa", None))
            return torch.zeros(x.shape, dtype=torch.int8), torch.zeros(x.shape[:-1] + (1,), dtype=torch.float32)

        monkeypatch.setattr("qqq_amd.attention.ops.dynamic_quant", dynamic_quant)
        monkeypatch.setattr(attn, "project_qkv", lambda xq, s1: (torch.zeros((xq.shape[0], h * d), dtype=torch.float16),
                                                                 torch.zeros((xq.shape[0], attn.num_key_value_heads * d), dtype=torch.float16),
                                                                 torch.zeros((xq.shape[0], attn.num_key_value_heads * d), dtype=torch.float16)))
        monkeypatch.setattr(attn.o_proj, "forward_int8", lambda aq, a1: torch.zeros((aq.shape[0], 256), dtype=torch.float16))

    def take(self):
        out, self.calls = self.calls, []
        return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_fuse_verify_routes_uniform_chunks_and_nothing_else(monkeypatch, dtype):
    from qqq_amd import PagedKVCache, QuantLlamaAttention

    kv8 = "_kv8" if dtype == torch.int8 else ""
    attn = QuantLlamaAttention(256, 4, 2, -1)  # G = 2, head_dim 64
    routes = _Routes(attn, monkeypatch)
    cache = PagedKVCache(1, 16, 2, 64, 16, dtype=dtype)
    for sid in ("a", "b"):
        cache.add(sid)

    def run(counts):
        step = cache.step(["a", "b"], counts)
        xq, s1 = torch.zeros((sum(counts), 256), dtype=torch.int8), torch.zeros((sum(counts), 1), dtype=torch.float32)
        out = attn.forward_int8(xq, s1, cache, step)
        assert out.shape == (sum(counts), 256)
        return step, routes.take()

    # without the flag: a uniform chunk goes to SDPA, or to the prefill kernel after fuse_prefill()
    assert run([4, 4])[1] == [("sdpa", None)]
    attn.fuse_prefill()
    step, calls = run([4, 4])
    assert calls == [("prefill_attention_paged" + kv8, step.max_len)]
    attn.fuse_verify()
    # with it: the uniform chunk takes the verify op with the step's T; everything else stays where it was
    step, calls = run([4, 4])
    assert calls == [("verify_attention_paged" + kv8, step.max_len, 4)]
    assert run([1, 1])[1][0][0] == "decode_attention_paged" + kv8  # a decode step
    assert run([4, 3])[1][0][0] == "prefill_attention_paged" + kv8  # ragged
    assert run([2, 2])[1][0][::2] == ("verify_attention_paged" + kv8, 2)
    assert run([16, 16])[1][0][:1] == ("verify_attention_paged" + kv8,) and routes.take() == []
    assert run([17, 17])[1][0][0] == "prefill_attention_paged" + kv8  # T = 17
    attn.unfuse_prefill()
    assert run([17, 17])[1] == [("sdpa", None)]  # too wide for the kernel, and no fuse_prefill(): SDPA, one dynamic_quant
    assert run([3, 3])[1][0][0] == "verify_attention_paged" + kv8
    attn.unfuse_verify()
    assert run([3, 3])[1] == [("sdpa", None)]
    # G * T > 64: eight query heads per KV head take chunks of up to 8 tokens
    wide = QuantLlamaAttention(512, 8, 1, -1).fuse_verify().fuse_prefill()  # G = 8
    routes = _Routes(wide, monkeypatch)
    monkeypatch.setattr(wide.o_proj, "forward_int8", lambda aq, a1: torch.zeros((aq.shape[0], 512), dtype=torch.float16))
    cache = PagedKVCache(1, 16, 1, 64, 16, dtype=dtype)
    cache.add("a")
    for t, want in ((8, "verify_attention_paged"), (9, "prefill_attention_paged")):
        step = cache.step(["a"], [t])
        wide.forward_int8(torch.zeros((t, 512), dtype=torch.int8), torch.zeros((t, 1), dtype=torch.float32), cache, step)
        assert routes.take()[0][0] == want + kv8, t


def test_spec_loop_constructor_accepts_either_flag():
    from qqq_amd import SpecDecodeLoop
    from test_step_cpu import _tiny_lm

    m = _tiny_lm()
    cache = m.new_cache(6, 16)
    with pytest.raises(RuntimeError, match="fuse_prefill.*fuse_verify"):
        SpecDecodeLoop(m, cache, rows=2, max_len=48, graph=False)
    m.fuse_verify()
    loop = SpecDecodeLoop(m, cache, rows=2, max_len=48, draft_len=3, graph=False)
    assert loop.group == 4 and loop.step.counts == [4, 4] and loop.step.start_pos is loop.start
    assert all(layer.self_attn._verify_tokens(loop.step) == 4 for layer in m.model.layers)
    m.unfuse_verify()
    with pytest.raises(RuntimeError, match="fuse_verify"):
        SpecDecodeLoop(m, cache, rows=2, max_len=48, graph=False)
    m.fuse_prefill()
    SpecDecodeLoop(m, cache, rows=2, max_len=48, graph=False)
