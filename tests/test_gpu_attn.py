"""rope_qkv, the attention module and the decoder layer on the GPU: bit-exact against the torch expression (tests/attn_ref.py) and the
composition of existing ops, incremental decoding against from-scratch runs, and transformers' fp16 LlamaDecoderLayer."""
import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16)


def _tables(dev, n, d, seed):
    # arbitrary fp16 tables (the kernel reads whatever it is given); both halves differ, so a half mix-up cannot pass
    g = torch.Generator(device=dev).manual_seed(seed)
    return ((torch.rand((n, d), generator=g, device=dev) * 2 - 1).half(), (torch.rand((n, d), generator=g, device=dev) * 2 - 1).half())


SENT = -1234.0  # a sentinel fp16 value in every cache slot the call must not touch


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,kvh", [(32, 32), (32, 8), (28, 4), (14, 2)])
def test_rope_qkv_bit_exact(dev, d, h, kvh):
    from qqq_amd import ops

    cap = 1400
    cos, sin = _tables(dev, 1500, d, seed=d + h)
    g = torch.Generator(device=dev).manual_seed(h * kvh + d)
    for b in (1, 3):
        for s in (1, 7, 300):
            for start in (0, 1000):
                m = b * s
                qkv = (torch.randn((m, (h + 2 * kvh) * d), generator=g, device=dev) * 4).half()
                qkv[0, :8] = torch.tensor([65504, -65504, 0, -0.0, 6e-8, -6e-8, 1e-4, 1], dtype=torch.float16)
                pos = (start + torch.arange(s, device=dev)).repeat(b)
                nq, nk = h * d, kvh * d
                views = (qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:])
                for fused in (True, False):
                    q, k, v = views if fused else tuple(t.contiguous() for t in views)
                    kc = torch.full((b, kvh, cap, d), SENT, dtype=torch.float16, device=dev)
                    vc = kc.clone()
                    q_out = ops.rope_qkv(q, k, v, cos, sin, pos, kc, vc)
                    assert q_out.shape == (b, h, s, d) and q_out.is_contiguous()
                    want_q = R.rope_rows(q, h, cos, sin, pos).reshape(b, s, h, d).transpose(1, 2)
                    assert torch.equal(_bits(q_out), _bits(want_q)), (d, h, kvh, b, s, start, fused)
                    want_k = R.rope_rows(k, kvh, cos, sin, pos).reshape(b, s, kvh, d).transpose(1, 2)
                    assert torch.equal(_bits(kc[:, :, start:start + s]), _bits(want_k)), (d, h, kvh, b, s, start, fused)
                    assert torch.equal(_bits(vc[:, :, start:start + s]), _bits(v.reshape(b, s, kvh, d).transpose(1, 2)))
                    for c in (kc, vc):  # every other slot untouched
                        assert bool((c[:, :, :start] == SENT).all()) and bool((c[:, :, start + s:] == SENT).all())


def test_rope_qkv_out_of_range_positions_write_nothing(dev):
    from qqq_amd import ops

    b, s, h, kvh, d, cap = 2, 6, 8, 2, 128, 64
    cos, sin = _tables(dev, 40, d, seed=3)  # table shorter than the cache: the limit is min(cap, table_len) = 40
    m = b * s
    q = torch.randn((m, h * d), device=dev).half()
    k = torch.randn((m, kvh * d), device=dev).half()
    v = torch.randn((m, kvh * d), device=dev).half()
    pos = torch.tensor([0, -1, 39, 40, 63, 64, 5, -(1 << 40), 1 << 40, 12, 41, 39], device=dev)
    kc = torch.full((b, kvh, cap, d), SENT, dtype=torch.float16, device=dev)
    vc = kc.clone()
    q_out = ops.rope_qkv(q, k, v, cos, sin, pos, kc, vc)
    ok = (pos >= 0) & (pos < 40)
    want_q = R.rope_rows(q, h, cos, sin, pos.clamp(0, 39)).reshape(b, s, h, d).transpose(1, 2)
    want_k = R.rope_rows(k, kvh, cos, sin, pos.clamp(0, 39)).reshape(b, s, kvh, d)
    okb = ok.reshape(b, s)
    assert torch.equal(_bits(q_out)[okb[:, None, :].expand(b, h, s)], _bits(want_q)[okb[:, None, :].expand(b, h, s)])
    kw, vw = kc.clone(), vc.clone()
    for t in range(m):
        if ok[t]:
            bi, p = t // s, int(pos[t])
            assert torch.equal(_bits(kc[bi, :, p]), _bits(want_k[bi, t % s]))
            assert torch.equal(_bits(vc[bi, :, p]), _bits(v[t].reshape(kvh, d)))
            kw[bi, :, p] = SENT
            vw[bi, :, p] = SENT
    assert bool((kw == SENT).all()) and bool((vw == SENT).all())  # nothing else was written


def _tr():
    return pytest.importorskip("transformers")


def test_rope_tables_equal_transformers_on_the_gpu(dev):
    tr = _tr()
    from transformers.models.llama import modeling_llama as ml

    from qqq_amd import QuantLlamaDecoderLayer

    l3 = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}
    for rope in ({"rope_type": "default", "rope_theta": 10000.0}, dict(l3, rope_theta=500000.0)):
        cfg = tr.LlamaConfig(hidden_size=4096, num_attention_heads=32, num_key_value_heads=8, intermediate_size=256,
                             max_position_embeddings=131072, rope_parameters=rope)
        emb = ml.LlamaRotaryEmbedding(cfg).to(dev)
        n = 8192
        tc, ts = emb(torch.zeros(1, dtype=torch.float16, device=dev), torch.arange(n, device=dev)[None])
        attn = QuantLlamaDecoderLayer.from_config(cfg, -1).self_attn.to(dev)
        cos, sin = attn.rope_tables(n)
        assert cos.device.type == "cuda"
        assert torch.equal(_bits(cos), _bits(tc[0])) and torch.equal(_bits(sin), _bits(ts[0])), rope["rope_type"]


def _make_ql(dev, K, N, group_size, bias, seed, scale=1.0):
    from qqq_amd import QuantLinear, pack as P

    g = torch.Generator(device=dev).manual_seed(seed)
    ql = QuantLinear(4, group_size, K, N, bias=bias).to(dev)
    if group_size != -1:
        codes = torch.randint(0, 16, (K, N), generator=g, dtype=torch.int8, device=dev)
        ql.s_group.copy_((torch.rand((K // 128, N), generator=g, device=dev) * 1.5 + 0.05).half())
    else:
        codes = torch.randint(-7, 8, (K, N), generator=g, dtype=torch.int8, device=dev)
    ql.B.copy_(P.pack_codes(codes, group_size != -1))
    ql.s_channel.copy_((torch.rand((1, N), generator=g, device=dev) * 2e-4 + 1e-5) * scale)
    if bias:
        ql.bias.copy_((torch.randn(N, generator=g, device=dev) * 0.1).half())
    return ql


def _make_layer(dev, hidden, heads, kvh, inter, gs, qwen2, seed):
    from qqq_amd import QuantLlamaDecoderLayer

    layer = QuantLlamaDecoderLayer(hidden, heads, kvh, inter, gs, qkv_bias=qwen2, o_bias=False, rms_norm_eps=1e-6,
                                   rope_theta=1e6 if qwen2 else 1e4).to(dev)
    a, d = layer.self_attn, hidden // heads
    a.q_proj = _make_ql(dev, hidden, heads * d, gs, qwen2, seed, scale=10.0)  # peaked softmax: a rope or head-layout error shows
    a.k_proj = _make_ql(dev, hidden, kvh * d, gs, qwen2, seed + 1, scale=10.0)
    a.v_proj = _make_ql(dev, hidden, kvh * d, gs, qwen2, seed + 2)
    a.o_proj = _make_ql(dev, heads * d, hidden, gs, False, seed + 3)
    m = layer.mlp
    m.gate_proj, m.up_proj, m.down_proj = (_make_ql(dev, hidden, inter, gs, False, seed + 4), _make_ql(dev, hidden, inter, gs, False, seed + 5),
                                           _make_ql(dev, inter, hidden, gs, False, seed + 6))
    for n in (layer.input_layernorm, layer.post_attention_layernorm):
        n.weight.data = (1 + 0.1 * torch.randn(hidden, device=dev)).half()
    return layer


def _attn_composition(attn, xq, s1, cache, start):
    """the attention from existing ops: the three forward_int8 GEMMs, torch rope on the module's tables, a torch cache write, the same
    SDPA call, dynamic_quant, o_proj"""
    from qqq_amd import ops

    b = cache.batch
    m = xq.shape[0]
    s = m // b
    h, kvh, d = attn.num_heads, attn.num_key_value_heads, attn.head_dim
    cos, sin = attn.rope_tables(cache.capacity)
    pos = (start + torch.arange(s, device=xq.device)).repeat(b)
    q, k, v = attn.q_proj.forward_int8(xq, s1), attn.k_proj.forward_int8(xq, s1), attn.v_proj.forward_int8(xq, s1)
    qr = R.rope_rows(q, h, cos, sin, pos).reshape(b, s, h, d).transpose(1, 2)
    kr = R.rope_rows(k, kvh, cos, sin, pos).reshape(b, s, kvh, d).transpose(1, 2)
    kc, vc = cache.k[attn.layer_idx], cache.v[attn.layer_idx]
    kc[:, :, start:start + s] = kr
    vc[:, :, start:start + s] = v.reshape(b, s, kvh, d).transpose(1, 2)
    o = R.sdpa(qr.contiguous(), kc, vc, start, d ** -0.5, kvh)
    aq, a1 = ops.dynamic_quant(o)
    return attn.o_proj.forward_int8(aq.reshape(m, -1), a1.reshape(m, 1))


def _layer_composition(layer, x, cache, start):
    from qqq_amd import ops

    n1, n2 = layer.input_layernorm, layer.post_attention_layernorm
    xq, s1 = ops.rmsnorm_quant(x, n1.weight, n1.variance_epsilon)
    a = _attn_composition(layer.self_attn, xq, s1, cache, start)
    h = x + a
    mq, ms = ops.rmsnorm_quant(h, n2.weight, n2.variance_epsilon)
    return h + layer.mlp.forward_int8(mq, ms)


SHAPES = {"llama": (1024, 8, 8, 2048, False), "llama_gqa": (1024, 8, 2, 2048, False), "qwen2": (896, 14, 2, 1024, True),
          "llama3_g8": (1024, 8, 1, 2048, False)}


@pytest.mark.parametrize("kind", list(SHAPES))
@pytest.mark.parametrize("gs", [-1, 128])
def test_attention_and_layer_equal_the_composition(dev, kind, gs):
    from qqq_amd import KVCache, ops

    hidden, heads, kvh, inter, qwen2 = SHAPES[kind]
    layer = _make_layer(dev, hidden, heads, kvh, inter, gs, qwen2, seed=11)
    attn = layer.self_attn
    b, cap = 2, 96
    d = hidden // heads
    for fused in (False, True):
        attn.fuse_qkv() if fused else attn.unfuse_qkv()
        c_mod, c_ref = KVCache(1, b, kvh, d, cap, dev), KVCache(1, b, kvh, d, cap, dev)
        c_lay, c_lref = KVCache(1, b, kvh, d, cap, dev), KVCache(1, b, kvh, d, cap, dev)
        start = 0
        for s in (13, 1, 1, 6):  # prefill, two decode steps, a chunk at start > 0
            x = torch.randn((b * s, hidden), device=dev).half()
            xq, s1 = ops.dynamic_quant(x)
            got = attn.forward_int8(xq, s1, c_mod, start)
            want = _attn_composition(attn, xq, s1, c_ref, start)
            assert torch.equal(_bits(got), _bits(want)), (kind, gs, fused, s, start)
            assert torch.equal(_bits(attn(x.reshape(b, s, hidden), c_mod, start)), _bits(want.reshape(b, s, hidden)))
            assert torch.equal(_bits(c_mod.k[0]), _bits(c_ref.k[0])) and torch.equal(_bits(c_mod.v[0]), _bits(c_ref.v[0]))
            x3 = x.reshape(b, s, hidden)
            got_l = layer(x3, c_lay, start)
            want_l = _layer_composition(layer, x, c_lref, start)
            assert got_l.shape == (b, s, hidden) and torch.equal(_bits(got_l.reshape(b * s, hidden)), _bits(want_l)), (kind, gs, fused, s)
            assert torch.isfinite(got_l).all()
            start += s


def test_incremental_decoding_matches_from_scratch_runs(dev):
    """Prefill 37, decode 5 single tokens, then a 9-token chunk: each step's last-token output against a fresh prefill of the whole
    sequence so far.  Everything before the attention core is row-wise and bit-identical; SDPA evaluates a 1-token or 9-token query with
    another kernel / reduction order than a full causal prefill, a few fp16 ulps of the attention output, which the per-token int8
    re-quantisation in front of o_proj can turn into one-code steps of s1 / 127 of a row's scale; the bound, 1e-3 of the output's norm,
    leaves room for several of them (measured on an MI355X: 0 at every decode step, 3.4e-7 for the 9-token chunk)."""
    from qqq_amd import KVCache

    hidden, heads, kvh, inter = 1024, 8, 2, 2048
    layer = _make_layer(dev, hidden, heads, kvh, inter, 128, False, seed=21).eval()
    b, cap, d = 2, 64, hidden // heads
    xs = torch.randn((b, 37 + 5 + 9, hidden), device=dev).half()
    cache = KVCache(1, b, kvh, d, cap, dev)
    start, worst = 0, 0.0
    for s in (37, 1, 1, 1, 1, 1, 9):
        step = layer(xs[:, start:start + s], cache, start)[:, -1]
        full = layer(xs[:, :start + s], KVCache(1, b, kvh, d, cap, dev), 0)[:, -1]
        rel = float((step.float() - full.float()).norm() / full.float().norm())
        worst = max(worst, rel)
        print(f"incremental step s={s} start={start}: relative L2 difference of the last token vs from scratch {rel:.2e}")
        assert torch.isfinite(step).all() and rel <= 1e-3, (s, start, rel)
        start += s
    print(f"incremental decoding: worst relative L2 difference {worst:.2e}")


def _fake_quant_linear(ql):
    """The fp16 weight [N, K] a QuantLinear was packed from (codes * scales), rebuilt from its packed tensors on the GPU."""
    K, N = ql.infeatures, ql.outfeatures
    eye = torch.eye(K, device=ql.B.device, dtype=torch.float16)
    # forward_int8 of unit rows with scale 1 reads one weight row per token: W[:, k] = GEMM(e_k)
    xq = (eye * 1).to(torch.int8)
    s1 = torch.ones((K, 1), device=ql.B.device)
    bias = ql.bias
    ql.bias = None
    try:
        w = ql.forward_int8(xq, s1)
    finally:
        ql.bias = bias
    return w.t().contiguous(), (None if bias is None else bias.clone())


@pytest.mark.parametrize("gqa", [False, True])
def test_layer_against_transformers_llama_decoder_layer(dev, gqa):
    """A transformers LlamaDecoderLayer in fp16 with the weights the QuantLinears hold (read back exactly: unit-row GEMMs) against the
    quantised layer.  The difference is the int8 per-token activation quantisation in front of the seven GEMMs: amax / 127 steps, about
    0.8 % of a Gaussian row's rms each, and the weights are compared after their fp16 rounding; the bound on the relative L2 error of the
    layer's update (out - hidden) is 5e-2 (measured on an MI355X: 2.7e-2 with 8 kv heads, 2.8e-2 with 2).  A head-layout or rope-layout error gives O(1)."""
    tr = _tr()
    from transformers.models.llama import modeling_llama as ml

    from qqq_amd import KVCache

    hidden, heads, kvh, inter = 1024, 8, (2 if gqa else 8), 2048
    d = hidden // heads
    layer = _make_layer(dev, hidden, heads, kvh, inter, -1, False, seed=31)
    cfg = tr.LlamaConfig(hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=kvh, intermediate_size=inter, rms_norm_eps=1e-6,
                         max_position_embeddings=4096, rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
    cfg._attn_implementation = "sdpa"
    ref = ml.LlamaDecoderLayer(cfg, layer_idx=0).to(dev).half().eval()
    with torch.no_grad():
        for name in ("q_proj", "k_proj", "v_proj", "o_proj"):
            w, _ = _fake_quant_linear(getattr(layer.self_attn, name))
            getattr(ref.self_attn, name).weight.copy_(w)
        for name in ("gate_proj", "up_proj", "down_proj"):
            w, _ = _fake_quant_linear(getattr(layer.mlp, name))
            getattr(ref.mlp, name).weight.copy_(w)
        ref.input_layernorm.weight.copy_(layer.input_layernorm.weight)
        ref.post_attention_layernorm.weight.copy_(layer.post_attention_layernorm.weight)
    emb = ml.LlamaRotaryEmbedding(cfg).to(dev)
    b, s = 2, 33
    x = torch.randn((b, s, hidden), device=dev).half()
    pos = torch.arange(s, device=dev)[None].expand(b, s)
    with torch.no_grad():
        out = ref(x, attention_mask=None, position_ids=pos, position_embeddings=emb(x, pos))
        want = out[0] if isinstance(out, tuple) else out
        got = layer(x, KVCache(1, b, kvh, d, 64, dev), 0)
    du, dw = (got.float() - x.float()), (want.float() - x.float())
    rel = float((du - dw).norm() / dw.norm())
    print(f"vs transformers LlamaDecoderLayer (gqa={gqa}): relative L2 error of the layer's update {rel:.2e}")
    assert torch.isfinite(got).all() and rel <= 5e-2, rel


@pytest.mark.parametrize("s", [1, 300])
def test_llama2_7b_shaped_layer(dev, s):
    from qqq_amd import KVCache

    hidden, heads, inter = 4096, 32, 11008
    layer = _make_layer(dev, hidden, heads, heads, inter, 128, False, seed=41)
    layer.self_attn.fuse_qkv()
    layer.mlp.fuse_gate_up()
    b, start, cap = 1, 64, 512
    c_mod, c_ref = KVCache(1, b, heads, 128, cap, dev), KVCache(1, b, heads, 128, cap, dev)
    for name in ("k", "v"):  # the same history in both caches
        past = torch.randn((b, heads, start, 128), device=dev).half()
        getattr(c_mod, name)[0][:, :, :start] = past
        getattr(c_ref, name)[0][:, :, :start] = past
    x = torch.randn((b, s, hidden), device=dev).half()
    got = layer(x, c_mod, start)
    want = _layer_composition(layer, x.reshape(-1, hidden), c_ref, start)
    assert torch.equal(_bits(got.reshape(-1, hidden)), _bits(want)) and torch.isfinite(got).all()


def test_rope_qkv_traces_under_torch_compile(dev):
    from qqq_amd import ops

    h, kvh, d, b, s, cap = 8, 2, 128, 2, 5, 32
    cos, sin = _tables(dev, cap, d, seed=9)

    def f(qkv, pos, kc, vc):
        nq, nk = h * d, kvh * d
        return ops.rope_qkv(qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:], cos, sin, pos, kc, vc) * 2

    qkv = torch.randn((b * s, (h + 2 * kvh) * d), device=dev).half()
    pos = (3 + torch.arange(s, device=dev)).repeat(b)
    ke, ve = torch.zeros((b, kvh, cap, d), dtype=torch.float16, device=dev), torch.zeros((b, kvh, cap, d), dtype=torch.float16, device=dev)
    kcm, vcm = ke.clone(), ve.clone()
    eager = f(qkv, pos, ke, ve)
    comp = torch.compile(f, fullgraph=True)(qkv, pos, kcm, vcm)
    assert torch.equal(_bits(eager), _bits(comp)) and torch.equal(_bits(ke), _bits(kcm)) and torch.equal(_bits(ve), _bits(vcm))
    assert bool(ke[:, :, 3:8].abs().sum() > 0)


def test_rope_qkv_hipgraph_replays_with_new_positions(dev):
    from qqq_amd import ops

    h, kvh, d, b, cap = 32, 8, 128, 4, 64
    cos, sin = _tables(dev, cap, d, seed=10)
    qkv = torch.randn((b, (h + 2 * kvh) * d), device=dev).half()
    nq, nk = h * d, kvh * d
    q, k, v = qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:]
    pos = torch.full((b,), 5, dtype=torch.int64, device=dev)
    kc = torch.full((b, kvh, cap, d), SENT, dtype=torch.float16, device=dev)
    vc = kc.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.rope_qkv(q, k, v, cos, sin, pos, kc, vc)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = ops.rope_qkv(q, k, v, cos, sin, pos, kc, vc)
    torch.cuda.current_stream().wait_stream(side)
    kc.fill_(SENT)
    vc.fill_(SENT)
    for p in (7, 40, 63):
        pos.fill_(p)
        qkv.copy_(torch.randn_like(qkv))
        graph.replay()
        torch.cuda.synchronize()
        pv = pos.clone()
        assert torch.equal(_bits(out), _bits(R.rope_rows(q, h, cos, sin, pv).reshape(b, 1, h, d).transpose(1, 2)))
        assert torch.equal(_bits(kc[:, :, p]), _bits(R.rope_rows(k, kvh, cos, sin, pv)))
        assert torch.equal(_bits(vc[:, :, p]), _bits(v.reshape(b, kvh, d)))
    written = torch.zeros(cap, dtype=torch.bool, device=dev)
    written[[7, 40, 63]] = True
    assert bool((kc[:, :, ~written] == SENT).all()) and bool((vc[:, :, ~written] == SENT).all())
