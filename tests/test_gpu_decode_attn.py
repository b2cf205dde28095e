"""The split-K decode attention (decode_attention, include/qqq_amd_decode.h) on the GPU: against a float64 attention over keys 0 ... pos, its
(xq, s1) against dynamic_quant of its own fp16 row, rows that must write nothing, torch.compile, hipGraph replay at new positions, and the
opt-in fuse_decode() path of the attention module and the decoder layer."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_attn import _bits, _fake_quant_linear, _make_layer, _tr

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (32, 8), (28, 4), (14, 2)]


def _chunk(dev, b, kvh, max_len):
    # the host's split rule (qqq_decode_attn): about four workgroups per CU, at most 32 splits, chunks a multiple of 128 keys
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    splits = max(1, min(-(-4 * cus // (b * kvh)), min(32, -(-max_len // 128))))
    return -(-(-(-max_len // splits)) // 128) * 128


def _ref64(q, kc, vc, pos, scale):
    """float64 attention of q [b, h, 1, d] over keys 0 ... pos[bi] of the caches -> [b, h, d]"""
    b, h, _, d = q.shape
    kvh = kc.shape[1]
    out = torch.empty((b, h, d), dtype=torch.float64, device=q.device)
    for bi in range(b):
        p = int(pos[bi])
        k = kc[bi, :, :p + 1].double().repeat_interleave(h // kvh, 0)
        v = vc[bi, :, :p + 1].double().repeat_interleave(h // kvh, 0)
        s = torch.einsum("hd,hkd->hk", q[bi, :, 0].double(), k) * scale
        out[bi] = torch.einsum("hk,hkd->hd", torch.softmax(s, -1), v)
    return out


def _sdpa(q, kc, vc, pos, scale):
    b, h, _, d = q.shape
    rows = [F.scaled_dot_product_attention(q[bi:bi + 1], kc[bi:bi + 1, :, :int(pos[bi]) + 1], vc[bi:bi + 1, :, :int(pos[bi]) + 1],
                                           scale=scale, enable_gqa=h != kc.shape[1]) for bi in range(b)]
    return torch.cat(rows).reshape(b, h, d)


def _errors(o, ref, vc, pos):
    """(worst relative L2 per (row, head), worst max |o - ref| / max |v| over the keys attended)"""
    b, h, d = ref.shape
    o = o.double().reshape(b, h, d)
    rel = ((o - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-30)).max().item()
    vmax = max(vc[bi, :, :int(pos[bi]) + 1].abs().max().item() for bi in range(b))
    return rel, (o - ref).abs().max().item() / vmax


def _check(q, kc, vc, pos, scale, what, **kw):
    from qqq_amd import ops

    xq, s1, o = ops.decode_attention(q, kc, vc, pos, scale, return_fp16=True, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(o).all(), what
    ref = _ref64(q, kc, vc, pos, scale)
    rel, mx = _errors(o, ref, vc, pos)
    srel, smx = _errors(_sdpa(q, kc, vc, pos, scale), ref, vc, pos)
    print(f"{what}: decode_attention rel L2 {rel:.2e}, max|err|/max|v| {mx:.2e} (2^-9 = {2 ** -9:.2e});  SDPA {srel:.2e}, {smx:.2e}")
    assert rel <= 1e-3 and mx <= 2 ** -9, (what, rel, mx)
    wq, ws = ops.dynamic_quant(o)
    assert torch.equal(xq, wq) and torch.equal(s1.view(torch.int32), ws.view(torch.int32)), what
    return o


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,kvh", SHAPES)
def test_decode_attention_against_float64(dev, d, h, kvh):
    b, cap = 3, 4160
    g = torch.Generator(device=dev).manual_seed(h * 7 + kvh + d)
    kc = torch.randn((b, kvh, cap, d), generator=g, device=dev).half()
    vc = torch.randn((b, kvh, cap, d), generator=g, device=dev).half()
    q = torch.randn((b, h, 1, d), generator=g, device=dev).half()
    c = _chunk(dev, b, kvh, cap)
    scale = d ** -0.5
    for p in [(0, 1, c - 1), (c, c + 1, 4095), (cap - 1, 17, 2 * c + 5)]:
        pos = torch.tensor(p, dtype=torch.int64, device=dev)
        _check(q, kc, vc, pos, scale, f"d={d} h={h} kvh={kvh} chunk={c} pos={p}")


@pytest.mark.parametrize("d", [64, 128])
def test_peaked_softmax_and_maximum_in_the_last_split(dev, d):
    h, kvh, b, cap = 32, 8, 2, 4096
    g = torch.Generator(device=dev).manual_seed(5 + d)
    kc = torch.randn((b, kvh, cap, d), generator=g, device=dev).half()
    vc = torch.randn((b, kvh, cap, d), generator=g, device=dev).half()
    q = torch.randn((b, h, 1, d), generator=g, device=dev).half()
    pos = torch.tensor([cap - 1, 3000], dtype=torch.int64, device=dev)
    for bi in range(b):  # the row's last key (in its last split) aligned with every query of its KV head: a near one-hot softmax
        p = int(pos[bi])
        for kh in range(kvh):
            qs = q[bi, kh * (h // kvh):(kh + 1) * (h // kvh), 0].float().sum(0)
            kc[bi, kh, p] = (qs / qs.norm() * 3 * math.sqrt(d)).half()
    _check(q, kc, vc, pos, d ** -0.5, f"peaked d={d}")
    # scores x30: the softmax stays finite and accurate
    _check(q, kc, vc, pos, 30 * d ** -0.5, f"scores x30 d={d}")
    q2 = (q.float() * 30).half()
    _check(q2, kc, vc, torch.tensor([cap - 1, 1], dtype=torch.int64, device=dev), d ** -0.5, f"q x30 d={d}")


SENT = -1234.0


def test_out_of_range_rows_and_the_cache_are_untouched(dev):
    from qqq_amd import _lib, ops

    h, kvh, d, b, cap, max_len = 32, 8, 128, 4, 512, 300
    kc = torch.randn((b, kvh, cap, d), device=dev).half()
    vc = torch.randn((b, kvh, cap, d), device=dev).half()
    k0, v0 = kc.clone(), vc.clone()
    q = torch.randn((b, h, 1, d), device=dev).half()
    pos = torch.tensor([-1, 299, 300, cap], dtype=torch.int64, device=dev)  # only row 1 is in [0, min(cap, max_len))
    o = torch.full((b, h * d), SENT, dtype=torch.float16, device=dev)
    xq = torch.full((b, h * d), 77, dtype=torch.int8, device=dev)
    s1 = torch.full((b, 1), SENT, dtype=torch.float32, device=dev)
    L = _lib.lib()
    nb = L.qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len)
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    err = L.qqq_decode_attn(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), pos.data_ptr(), d ** -0.5, o.data_ptr(), xq.data_ptr(),
                            s1.data_ptr(), ws.data_ptr(), nb, b, h, kvh, d, cap, max_len, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert err == 0, _lib.last_error()
    for bi in (0, 2, 3):
        assert bool((o[bi] == SENT).all()) and bool((xq[bi] == 77).all()) and float(s1[bi]) == SENT, bi
    assert torch.equal(_bits(kc), _bits(k0)) and torch.equal(_bits(vc), _bits(v0))
    xw, sw, ow = ops.decode_attention(q[1:2], kc[1:2], vc[1:2], pos[1:2], d ** -0.5, max_len=max_len, return_fp16=True)
    assert torch.equal(_bits(o[1:2]), _bits(ow)) and torch.equal(xq[1:2], xw) and torch.equal(s1[1:2], sw)


def test_decode_attention_traces_under_torch_compile(dev):
    from qqq_amd import ops

    h, kvh, d, b, cap = 28, 4, 128, 2, 256
    kc, vc = torch.randn((b, kvh, cap, d), device=dev).half(), torch.randn((b, kvh, cap, d), device=dev).half()
    q = torch.randn((b, h, 1, d), device=dev).half()
    pos = torch.tensor([200, 31], dtype=torch.int64, device=dev)

    def f(q, kc, vc, pos):
        xq, s1, o = ops.decode_attention(q * 1, kc, vc, pos, d ** -0.5, return_fp16=True)
        return xq, s1 * 2, o

    eager = f(q, kc, vc, pos)
    comp = torch.compile(f, fullgraph=True)(q, kc, vc, pos)
    for e, c in zip(eager, comp):
        assert torch.equal(e.view(torch.int8), c.view(torch.int8))


def test_decode_attention_hipgraph_replays_at_new_positions(dev):
    from qqq_amd import ops

    h, kvh, d, b, cap = 32, 8, 128, 2, 2048
    kc, vc = torch.randn((b, kvh, cap, d), device=dev).half(), torch.randn((b, kvh, cap, d), device=dev).half()
    q = torch.randn((b, h, 1, d), device=dev).half()
    pos = torch.tensor([5, 9], dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.decode_attention(q, kc, vc, pos, d ** -0.5, max_len=cap, return_fp16=True)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = ops.decode_attention(q, kc, vc, pos, d ** -0.5, max_len=cap, return_fp16=True)
    torch.cuda.current_stream().wait_stream(side)
    for p in ((7, 1000), (1500, 0), (cap - 1, 129)):
        pos.copy_(torch.tensor(p, device=dev))
        q.copy_(torch.randn_like(q))
        graph.replay()
        torch.cuda.synchronize()
        want = ops.decode_attention(q, kc, vc, pos, d ** -0.5, max_len=cap, return_fp16=True)
        for g_, w_ in zip(out, want):
            assert torch.equal(g_.view(torch.int8), w_.view(torch.int8)), p


def _decode_composition(attn, xq, s1, cache, start):
    """project_qkv -> rope_qkv -> decode_attention -> o_proj.forward_int8"""
    from qqq_amd import ops

    cos, sin = attn.rope_tables(cache.capacity)
    q, k, v = attn.project_qkv(xq, s1)
    pos = cache.positions(start, 1)
    kc, vc = cache.k[attn.layer_idx], cache.v[attn.layer_idx]
    q_out = ops.rope_qkv(q, k, v, cos, sin, pos, kc, vc)
    aq, a1 = ops.decode_attention(q_out, kc, vc, pos, attn.scaling, max_len=start + 1)
    return attn.o_proj.forward_int8(aq, a1)


MODULE_SHAPES = {"llama": (1024, 8, 8, 2048, False), "llama_gqa": (1024, 8, 2, 2048, False), "qwen2": (896, 14, 2, 1024, True),
                 "llama3_g8": (1024, 8, 1, 2048, False)}


@pytest.mark.parametrize("kind", list(MODULE_SHAPES))
def test_fused_decode_module_equals_the_composition(dev, kind):
    from qqq_amd import KVCache, ops

    hidden, heads, kvh, inter, qwen2 = MODULE_SHAPES[kind]
    layer = _make_layer(dev, hidden, heads, kvh, inter, 128, qwen2, seed=51)
    attn = layer.self_attn
    assert layer.fuse_decode() is layer and layer.decode_fused and attn.decode_fused
    b, cap, d = 2, 160, hidden // heads
    for fused_qkv in (False, True):
        attn.fuse_qkv() if fused_qkv else attn.unfuse_qkv()
        c_mod, c_ref, c_sdpa = (KVCache(1, b, kvh, d, cap, dev) for _ in range(3))
        start = 0
        for s in (130, 1, 1, 5, 1):  # prefill (SDPA), decode steps (the kernel), a chunk (SDPA), a decode step
            x = torch.randn((b * s, hidden), device=dev).half()
            xq, s1 = ops.dynamic_quant(x)
            got = attn.forward_int8(xq, s1, c_mod, start)
            attn.unfuse_decode()
            plain = attn.forward_int8(xq, s1, c_sdpa, start)
            attn.fuse_decode()
            if s == 1:
                want = _decode_composition(attn, xq, s1, c_ref, start)
                assert torch.equal(_bits(got), _bits(want)), (kind, fused_qkv, start)
                rel = float((got.float() - plain.float()).norm() / plain.float().norm())
                print(f"{kind} fused_qkv={fused_qkv} decode at {start}: relative L2 vs the SDPA path {rel:.2e}")
                assert rel <= 1e-2, rel
            else:
                attn.forward_int8(xq, s1, c_ref, start)
                assert torch.equal(_bits(got), _bits(plain)), (kind, fused_qkv, s)  # s > 1 keeps the SDPA path
            assert torch.equal(_bits(c_mod.k[0]), _bits(c_sdpa.k[0])) and torch.equal(_bits(c_mod.v[0]), _bits(c_sdpa.v[0]))
            start += s


def test_fused_decode_layer_steps_against_sdpa_and_from_scratch(dev):
    from qqq_amd import KVCache

    hidden, heads, kvh, inter = 1024, 8, 2, 2048
    layer = _make_layer(dev, hidden, heads, kvh, inter, 128, False, seed=61).eval()
    b, cap, d = 2, 600, hidden // heads
    xs = torch.randn((b, 520 + 6, hidden), device=dev).half()
    c_fused, c_plain = KVCache(1, b, kvh, d, cap, dev), KVCache(1, b, kvh, d, cap, dev)
    layer.fuse_decode()
    layer(xs[:, :520], c_fused, 0)
    layer.unfuse_decode()
    layer(xs[:, :520], c_plain, 0)
    worst = 0.0
    for start in range(520, 526):
        layer.fuse_decode()
        step = layer(xs[:, start:start + 1], c_fused, start)[:, -1]
        layer.unfuse_decode()
        plain = layer(xs[:, start:start + 1], c_plain, start)[:, -1]
        full = layer(xs[:, :start + 1], KVCache(1, b, kvh, d, cap, dev), 0)[:, -1]
        r1 = float((step.float() - plain.float()).norm() / plain.float().norm())
        r2 = float((step.float() - full.float()).norm() / full.float().norm())
        worst = max(worst, r1, r2)
        print(f"fused decode step at {start}: relative L2 vs the SDPA path {r1:.2e}, vs from scratch {r2:.2e}")
        assert torch.isfinite(step).all() and r1 <= 1e-2 and r2 <= 1e-2, (start, r1, r2)
    print(f"fused decode steps: worst relative L2 {worst:.2e}")


@pytest.mark.parametrize("gqa", [False, True])
def test_fused_decode_layer_against_transformers_llama_decoder_layer(dev, gqa):
    """transformers' fp16 LlamaDecoderLayer over the whole sequence (causal) against the quantised layer run as a 32-token prefill and 8
    decode steps with fuse_decode(): the same 5e-2 bound on the relative L2 error of the layer's update as tests/test_gpu_attn.py."""
    tr = _tr()
    from transformers.models.llama import modeling_llama as ml

    from qqq_amd import KVCache

    hidden, heads, kvh, inter = 1024, 8, (2 if gqa else 8), 2048
    d = hidden // heads
    layer = _make_layer(dev, hidden, heads, kvh, inter, -1, False, seed=71)
    cfg = tr.LlamaConfig(hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=kvh, intermediate_size=inter, rms_norm_eps=1e-6,
                         max_position_embeddings=4096, rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
    cfg._attn_implementation = "sdpa"
    ref = ml.LlamaDecoderLayer(cfg, layer_idx=0).to(dev).half().eval()
    with torch.no_grad():
        for name in ("q_proj", "k_proj", "v_proj", "o_proj"):
            getattr(ref.self_attn, name).weight.copy_(_fake_quant_linear(getattr(layer.self_attn, name))[0])
        for name in ("gate_proj", "up_proj", "down_proj"):
            getattr(ref.mlp, name).weight.copy_(_fake_quant_linear(getattr(layer.mlp, name))[0])
        ref.input_layernorm.weight.copy_(layer.input_layernorm.weight)
        ref.post_attention_layernorm.weight.copy_(layer.post_attention_layernorm.weight)
    emb = ml.LlamaRotaryEmbedding(cfg).to(dev)
    b, pre, steps = 2, 32, 8
    s = pre + steps
    x = torch.randn((b, s, hidden), device=dev).half()
    pos = torch.arange(s, device=dev)[None].expand(b, s)
    layer.fuse_decode()
    with torch.no_grad():
        out = ref(x, attention_mask=None, position_ids=pos, position_embeddings=emb(x, pos))
        want = (out[0] if isinstance(out, tuple) else out)[:, pre:]
        cache = KVCache(1, b, kvh, d, 64, dev)
        layer(x[:, :pre], cache, 0)
        got = torch.cat([layer(x[:, t:t + 1], cache, t) for t in range(pre, s)], dim=1)
    du, dw = (got.float() - x[:, pre:].float()), (want.float() - x[:, pre:].float())
    rel = float((du - dw).norm() / dw.norm())
    print(f"fused decode vs transformers LlamaDecoderLayer (gqa={gqa}): relative L2 error of the decode steps' update {rel:.2e}")
    assert torch.isfinite(got).all() and rel <= 5e-2, rel
