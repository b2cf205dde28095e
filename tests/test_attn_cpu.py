"""Attention block without a GPU: the C-ABI of include/qqq_amd_attn.h (declared set, export, argument checks before any launch), the rope
kernel's resources in the gfx950 code object, the modules' reference-keyed state-dicts, the rope tables and the torch restatement
(tests/attn_ref.py) against transformers when it is installed."""
import gc
import os
import sys
import weakref

import pytest
import torch

import attn_ref as R

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


def test_header_declares_rope_qkv_and_the_library_exports_it(L):
    names = _declared("qqq_amd_attn.h")
    assert names == {"qqq_rope_qkv"}
    assert hasattr(L, "qqq_rope_qkv")
    assert L.qqq_amd_abi_version() == 4


# fake device addresses with the alignment the entry point asks for (16 bytes; pos 8): the calls below must fail in the checks
A16, A8 = 0x1000, 0x2008


def _rope(L, q=A16, ldq=4096, k=A16, ldk=1024, v=A16, ldv=1024, cos=A16, sin=A16, tl=4096, pos=A8, qo=A16, kc=A16, vc=A16, b=2, s=3,
          h=32, kvh=8, d=128, cap=4096):
    return L.qqq_rope_qkv(q, ldq, k, ldk, v, ldv, cos, sin, tl, pos, qo, kc, vc, b, s, h, kvh, d, cap, 0, None)


BAD = [dict(q=None), dict(k=None), dict(v=None), dict(cos=None), dict(sin=None), dict(pos=None), dict(qo=None), dict(kc=None),
       dict(vc=None), dict(q=A16 + 8), dict(k=A16 + 2), dict(v=A16 + 4), dict(cos=A16 + 8), dict(sin=A16 + 2), dict(pos=A8 + 4),
       dict(qo=A16 + 8), dict(kc=A16 + 2), dict(vc=A16 + 8), dict(ldq=4088), dict(ldk=1016), dict(ldv=1000), dict(ldq=4100),
       dict(ldk=1028), dict(ldv=1026), dict(d=72, ldq=32 * 72, ldk=8 * 72, ldv=8 * 72), dict(d=8, ldq=256, ldk=64, ldv=64),
       dict(d=272, ldq=32 * 272, ldk=8 * 272, ldv=8 * 272), dict(d=0), dict(h=30, ldq=30 * 128), dict(kvh=0), dict(h=0), dict(b=-1),
       dict(s=-1), dict(h=-32), dict(kvh=-8), dict(d=-128), dict(cap=-1), dict(tl=-1), dict(h=8192, kvh=8192, ldq=1 << 20, ldk=1 << 20,
       ldv=1 << 20), dict(b=1 << 16, s=1 << 16)]


@pytest.mark.parametrize("kw", BAD)
def test_rope_qkv_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _rope(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_rope_qkv:")


def test_rope_qkv_accepts_the_good_call_shapes_in_its_checks(L):
    # the same checks with every argument good would launch: here only the no-token calls may be made (no GPU)
    assert _rope(L, b=0) == 0 and _rope(L, s=0) == 0
    assert L.qqq_rope_qkv(None, 0, None, 0, None, 0, None, None, 0, None, None, None, None, 0, 5, 32, 8, 128, 0, 0, None) == 0
    assert L.qqq_rope_qkv(None, 0, None, 0, None, 0, None, None, 0, None, None, None, None, 3, 0, 0, 0, 0, 0, 0, None) == 0


def test_rope_kernel_in_the_code_object_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = [k for k in code_object.kernels(build.LIB) if k["demangled"].startswith("qqq_rope_qkv_kernel<")]
    assert [k["demangled"] for k in ks] == ["qqq_rope_qkv_kernel<128>"]
    for k in ks:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["group_segment_fixed_size"] == 0, k  # no LDS
        assert k["max_flat_workgroup_size"] == 128


def test_cpu_tensors_raise():
    from qqq_amd import ops

    m, d = 3, 64
    q, k = torch.zeros((m, 4 * d), dtype=torch.float16), torch.zeros((m, 2 * d), dtype=torch.float16)
    cos = torch.zeros((16, d), dtype=torch.float16)
    cache = torch.zeros((1, 2, 16, d), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rope_qkv(q, k, k, cos, cos, torch.arange(m), cache, cache.clone())
    from qqq_amd import KVCache, QuantLlamaAttention

    attn = QuantLlamaAttention(256, 4, 2, -1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        attn(torch.zeros((1, 3, 256), dtype=torch.float16), KVCache(1, 1, 2, 64, 16), 0)


def _random_sd(module, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.randint(-2**31, 2**31 - 1, v.shape, generator=g, dtype=torch.int32) if v.dtype == torch.int32
                else torch.rand(v.shape, generator=g).to(v.dtype)) for k, v in module.state_dict().items()}


def _reference_layer(hidden, heads, kvh, inter, gs, qkv_bias, o_bias):
    """A module tree with the reference's Quantized{Llama,Qwen2}DecoderLayer keys: QuantLinears named as there, LlamaRMSNorm weights."""
    from qqq_amd import QuantLinear

    d = hidden // heads
    attn = torch.nn.Module()
    attn.q_proj = QuantLinear(4, gs, hidden, heads * d, bias=qkv_bias)
    attn.k_proj = QuantLinear(4, gs, hidden, kvh * d, bias=qkv_bias)
    attn.v_proj = QuantLinear(4, gs, hidden, kvh * d, bias=qkv_bias)
    attn.o_proj = QuantLinear(4, gs, hidden, hidden, bias=o_bias)
    mlp = torch.nn.Module()
    mlp.gate_proj = QuantLinear(4, gs, hidden, inter, bias=False)
    mlp.up_proj = QuantLinear(4, gs, hidden, inter, bias=False)
    mlp.down_proj = QuantLinear(4, gs, inter, hidden, bias=False)
    layer = torch.nn.Module()
    layer.self_attn, layer.mlp = attn, mlp
    layer.input_layernorm, layer.post_attention_layernorm = torch.nn.Module(), torch.nn.Module()
    layer.input_layernorm.weight = torch.nn.Parameter(torch.ones(hidden))
    layer.post_attention_layernorm.weight = torch.nn.Parameter(torch.ones(hidden))
    return layer


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _llama_cfg(bias=False, **kw):
    c = dict(model_type="llama", hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512, rms_norm_eps=1e-5,
             hidden_act="silu", attention_bias=bias, rope_theta=10000.0, rope_scaling=None)
    c.update(kw)
    return _Cfg(**c)


@pytest.mark.parametrize("kind", ["llama", "llama_bias", "qwen2"])
@pytest.mark.parametrize("gs", [-1, 128])
def test_decoder_layer_loads_reference_keyed_state_dicts_strictly(kind, gs):
    from qqq_amd import QuantLlamaDecoderLayer

    qkv_bias, o_bias = {"llama": (False, False), "llama_bias": (True, True), "qwen2": (True, False)}[kind]
    ref = _reference_layer(256, 4, 2, 512, gs, qkv_bias, o_bias)
    sd = _random_sd(ref, seed=3)
    if kind == "qwen2":
        cfg = _llama_cfg(model_type="qwen2", use_sliding_window=False)
    else:
        cfg = _llama_cfg(bias=qkv_bias)
    layer = QuantLlamaDecoderLayer.from_config(cfg, gs, layer_idx=0)
    assert set(layer.state_dict()) == set(sd)
    layer.load_state_dict(sd, strict=True)
    for k, v in layer.state_dict().items():
        assert torch.equal(v, sd[k].to(v.dtype)), k
    # fuse_qkv() keeps the state-dict as it was; loading drops the fused copy
    layer.self_attn.fuse_qkv()
    assert layer.self_attn.qkv_fused and layer.self_attn._qkv.outfeatures == (4 + 2 * 2) * 64
    sd2 = layer.state_dict()
    assert set(sd2) == set(sd) and all(torch.equal(sd2[k], sd[k].to(sd2[k].dtype)) for k in sd)
    assert layer.self_attn._qkv.B.data_ptr() not in {t.data_ptr() for t in sd2.values()}
    layer.load_state_dict(sd, strict=True)
    assert not layer.self_attn.qkv_fused


def test_from_config_reads_both_transformers_styles_and_rejects_the_unsupported():
    from qqq_amd import QuantLlamaDecoderLayer

    l3 = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}
    a = QuantLlamaDecoderLayer.from_config(_llama_cfg(rope_theta=500000.0, rope_scaling=dict(l3)), -1).self_attn
    b = QuantLlamaDecoderLayer.from_config(_llama_cfg(rope_parameters=dict(l3, rope_theta=500000.0)), -1).self_attn
    c = QuantLlamaDecoderLayer.from_config(_llama_cfg(rope_theta=500000.0), -1).self_attn
    assert torch.equal(a.inv_freq, b.inv_freq) and not torch.equal(a.inv_freq, c.inv_freq)
    assert a.num_heads == 4 and a.num_key_value_heads == 2 and a.head_dim == 64 and a.q_proj.bias is None
    q = QuantLlamaDecoderLayer.from_config(_llama_cfg(model_type="qwen2", use_sliding_window=False), -1).self_attn
    assert q.q_proj.bias is not None and q.k_proj.bias is not None and q.v_proj.bias is not None and q.o_proj.bias is None
    with pytest.raises(NotImplementedError):
        QuantLlamaDecoderLayer.from_config(_llama_cfg(model_type="qwen2", use_sliding_window=True), -1)
    for bad in ({"rope_type": "linear", "factor": 2.0}, {"type": "dynamic", "factor": 2.0}, {"rope_type": "yarn", "factor": 4.0}):
        with pytest.raises(NotImplementedError):
            QuantLlamaDecoderLayer.from_config(_llama_cfg(rope_scaling=bad), -1)
    with pytest.raises(NotImplementedError):
        QuantLlamaDecoderLayer.from_config(_llama_cfg(rope_parameters={"rope_type": "longrope", "rope_theta": 1e4}), -1)


def test_layer_is_freed_without_the_cycle_collector():
    from qqq_amd import QuantLlamaDecoderLayer

    gc.collect()
    gc.disable()
    try:
        layer = QuantLlamaDecoderLayer(256, 4, 2, 512, 128)
        layer.self_attn.fuse_qkv()
        layer.mlp.fuse_gate_up()
        layer.self_attn.rope_tables(64)
        ref = weakref.ref(layer)
        fused = weakref.ref(layer.self_attn._qkv)
        del layer
        assert ref() is None and fused() is None
    finally:
        gc.enable()


def test_kv_cache_layout_and_positions():
    from qqq_amd import KVCache

    c = KVCache(2, 3, 4, 64, 100)
    assert len(c.k) == 2 and c.k[0].shape == (3, 4, 100, 64) and c.k[1].dtype == torch.float16
    assert c.nbytes == 4 * 2 * 3 * 4 * 100 * 64 == sum(t.numel() * t.element_size() for t in c.k + c.v)
    assert c.positions(7, 1).tolist() == [7, 7, 7]
    assert c.positions(5, 3).tolist() == [5, 6, 7] * 3
    assert KVCache(1, 1, 1, 16, 50).positions(10, 4).tolist() == [10, 11, 12, 13]


def _rope_cfg(rope):
    tr = pytest.importorskip("transformers")
    kw = dict(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, intermediate_size=256, max_position_embeddings=4096)
    try:
        return tr.LlamaConfig(rope_parameters=dict(rope, rope_theta=500000.0), **kw)
    except TypeError:
        r = {k: v for k, v in rope.items() if k != "rope_type" or v != "default"}
        return tr.LlamaConfig(rope_theta=500000.0, rope_scaling=(r or None), **kw)


LLAMA3 = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 256}


@pytest.mark.parametrize("rope", [{"rope_type": "default"}, LLAMA3], ids=["default", "llama3"])
def test_rope_tables_equal_transformers_on_cpu(rope):
    from transformers.models.llama import modeling_llama as ml

    from qqq_amd import QuantLlamaDecoderLayer

    cfg = _rope_cfg(rope)
    emb = ml.LlamaRotaryEmbedding(cfg)
    n = 2000
    x = torch.zeros(1, dtype=torch.float16)
    tc, ts = emb(x, torch.arange(n)[None])
    attn = QuantLlamaDecoderLayer.from_config(cfg, -1).self_attn
    assert torch.equal(attn.inv_freq, emb.inv_freq)
    cos, sin = attn.rope_tables(n)
    assert cos.dtype == torch.float16 and cos.shape == (n, 128)
    assert torch.equal(cos.view(torch.int16), tc[0].view(torch.int16)) and torch.equal(sin.view(torch.int16), ts[0].view(torch.int16))


def test_restatement_rotary_equals_transformers():
    ml = pytest.importorskip("transformers.models.llama.modeling_llama")
    g = torch.Generator().manual_seed(5)
    b, h, kvh, s, d = 2, 4, 2, 9, 64
    q = (torch.randn((b, h, s, d), generator=g) * 3).half()
    k = (torch.randn((b, kvh, s, d), generator=g) * 3).half()
    cos = torch.rand((b, s, d), generator=g).half()
    sin = torch.rand((b, s, d), generator=g).half()
    tq, tk = ml.apply_rotary_pos_emb(q, k, cos, sin)
    assert torch.equal(R.apply_rotary(q, cos, sin).view(torch.int16), tq.view(torch.int16))
    assert torch.equal(R.apply_rotary(k, cos, sin).view(torch.int16), tk.view(torch.int16))
    # the per-row form the kernel tests use
    rows = q.transpose(1, 2).reshape(b * s, h * d)
    pos = torch.arange(s).repeat(b)
    table_c, table_s = cos[0], sin[0]
    got = R.rope_rows(rows, h, table_c, table_s, pos).reshape(b, s, h, d).transpose(1, 2)
    want = R.apply_rotary(q, table_c[None].expand(b, s, d), table_s[None].expand(b, s, d))
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def _lin(x, wb):
    return torch.nn.functional.linear(x, *wb)


@pytest.mark.parametrize("start", [0, 5])
def test_restatement_attention_equals_transformers_llama_attention(start):
    ml = pytest.importorskip("transformers.models.llama.modeling_llama")
    from qqq_amd.attention import rope_inv_freq, rope_tables

    torch.manual_seed(6)
    hidden, h, kvh, s, b = 256, 4, 2, 7, 2
    d = hidden // h
    cfg = _rope_cfg({"rope_type": "default"})
    cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim = hidden, h, kvh, d
    cfg._attn_implementation = "sdpa"
    attn = ml.LlamaAttention(cfg, layer_idx=0).eval()
    w = {n: (getattr(attn, f"{n}_proj").weight.detach(), None) for n in "qkvo"}
    cos, sin = rope_tables(*rope_inv_freq(d, 500000.0), 64, "cpu", dtype=torch.float32)
    x = torch.randn((b, start + s, hidden))
    want, _, _ = R.attention(x, w, h, kvh, cos, sin)
    pos = torch.arange(start + s)[None].expand(b, -1)
    with torch.no_grad():
        got, _ = attn(x, position_embeddings=(cos[pos], sin[pos]), attention_mask=None)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-5)
    if start:
        # a chunk at start > 0 on top of the first `start` tokens' k / v is the tail of the full run ...
        _, kp, vp = R.attention(x[:, :start], w, h, kvh, cos, sin)
        tail, _, _ = R.attention(x[:, start:], w, h, kvh, cos, sin, start=start, k_past=kp, v_past=vp)
        assert torch.allclose(tail, want[:, start:], rtol=1e-4, atol=1e-5)
        # ... and so is the module's SDPA call with its bottom-right causal mask
        c, sn = cos[:start + s][None], sin[:start + s][None]
        q = R.apply_rotary(_lin(x, w["q"]).view(b, -1, h, d).transpose(1, 2), c, sn)
        k = R.apply_rotary(_lin(x, w["k"]).view(b, -1, kvh, d).transpose(1, 2), c, sn)
        v = _lin(x, w["v"]).view(b, -1, kvh, d).transpose(1, 2)
        o = R.sdpa(q[:, :, start:], k, v, start, d ** -0.5, kvh)
        assert torch.allclose(_lin(o, w["o"]), want[:, start:], rtol=1e-4, atol=1e-5)
