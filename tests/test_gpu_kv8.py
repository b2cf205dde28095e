"""The int8 KV cache on the GPU (include/qqq_amd_kv8.h): rope_qkv_kv8 bit for bit against rope_qkv + dynamic_quant of every cached head row,
decode_attention_kv8 against a float64 attention over the exactly dequantised cache, rows that must write nothing, torch.compile, hipGraph
replay, and the attention module / decoder layer with KVCache(dtype=torch.int8)."""
import math

import pytest
import torch
import torch.nn.functional as F

import kv8_ref as K8
from test_gpu_attn import _bits, _fake_quant_linear, _make_layer, _tables, _tr
from test_gpu_decode_attn import _chunk

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (32, 8), (28, 4), (14, 2)]
SENT = -1234.0  # fp16 / f32 sentinel; 77 is the int8 one


def _i32(t):
    return t.contiguous().view(torch.int32)


def _empty_cache(dev, b, kvh, cap, d):
    kc = torch.full((b, kvh, cap, d), 77, dtype=torch.int8, device=dev)
    ks = torch.full((b, kvh, cap), SENT, dtype=torch.float32, device=dev)
    return kc, kc.clone(), ks, ks.clone()


# ---- rope_qkv_kv8

@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,kvh", SHAPES)
def test_rope_qkv_kv8_bit_exact(dev, d, h, kvh):
    from qqq_amd import ops

    cap = 1200
    cos, sin = _tables(dev, 1300, d, seed=d + h)
    g = torch.Generator(device=dev).manual_seed(h * kvh + d)
    for b in (1, 3):
        for s in (1, 7, 130):
            for start in (0, 1000):
                m = b * s
                # per-token amplitudes over many binades, so scales differ from row to row
                amp = torch.exp2(torch.randint(-8, 5, (m, 1), generator=g, device=dev).float())
                qkv = (torch.randn((m, (h + 2 * kvh) * d), generator=g, device=dev) * amp).half()
                nq, nk = h * d, kvh * d
                qkv[0, nq:nq + 8] = torch.tensor([30000, -30000, 0, -0.0, 6e-8, -6e-8, 1e-4, 1], dtype=torch.float16)  # in k's head 0
                qkv[0, nq + nk:nq + nk + 2] = torch.tensor([65504, -65504], dtype=torch.float16)  # in v's head 0
                qkv[m - 1, nq + nk:nq + nk + d] = 0  # an all-zero v head row: zero codes, zero scale
                if kvh > 1:
                    qkv[m - 1, nq + nk + d:nq + nk + 2 * d] = 6e-8  # a v head row whose scale rounds to zero
                pos = (start + torch.arange(s, device=dev)).repeat(b)
                views = (qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:])
                for fused in (True, False):
                    q, k, v = views if fused else tuple(t.contiguous() for t in views)
                    kc16 = torch.full((b, kvh, cap, d), SENT, dtype=torch.float16, device=dev)
                    vc16 = kc16.clone()
                    want_q = ops.rope_qkv(q, k, v, cos, sin, pos, kc16, vc16)
                    kc, vc, ks, vs = _empty_cache(dev, b, kvh, cap, d)
                    q_out = ops.rope_qkv_kv8(q, k, v, cos, sin, pos, kc, vc, ks, vs)
                    what = (d, h, kvh, b, s, start, fused)
                    assert q_out.shape == (b, h, s, d) and q_out.is_contiguous()
                    assert torch.equal(_bits(q_out), _bits(want_q)), what
                    sl = slice(start, start + s)
                    for codes, scales, c16 in ((kc, ks, kc16), (vc, vs, vc16)):
                        wc, wsc = K8.quant_rows_op(c16[:, :, sl])
                        assert torch.equal(codes[:, :, sl], wc), what
                        assert torch.equal(_i32(scales[:, :, sl]), _i32(wsc)), what
                        # every other slot untouched
                        assert bool((codes[:, :, :start] == 77).all()) and bool((codes[:, :, start + s:] == 77).all()), what
                        assert bool((scales[:, :, :start] == SENT).all()) and bool((scales[:, :, start + s:] == SENT).all()), what


def test_rope_qkv_kv8_out_of_range_positions_write_nothing(dev):
    from qqq_amd import ops

    b, s, h, kvh, d, cap = 2, 6, 8, 2, 128, 64
    cos, sin = _tables(dev, 40, d, seed=3)  # table shorter than the cache: the limit is min(cap, table_len) = 40
    m = b * s
    q = torch.randn((m, h * d), device=dev).half()
    k = torch.randn((m, kvh * d), device=dev).half()
    v = torch.randn((m, kvh * d), device=dev).half()
    pos = torch.tensor([0, -1, 39, 40, 63, 64, 5, -(1 << 40), 1 << 40, 12, 41, 39], device=dev)
    kc16 = torch.full((b, kvh, cap, d), SENT, dtype=torch.float16, device=dev)
    vc16 = kc16.clone()
    want_q = ops.rope_qkv(q, k, v, cos, sin, pos, kc16, vc16)
    kc, vc, ks, vs = _empty_cache(dev, b, kvh, cap, d)
    q_out = torch.ops.qqq_amd.rope_qkv_kv8(q, k, v, cos, sin, pos, kc, vc, ks, vs)  # the registered op, eagerly
    okb = ((pos >= 0) & (pos < 40)).reshape(b, s)
    sel = okb[:, None, :].expand(b, h, s)
    assert torch.equal(_bits(q_out)[sel], _bits(want_q)[sel])
    written = torch.zeros((b, kvh, cap), dtype=torch.bool, device=dev)
    for t in range(m):
        if okb.reshape(-1)[t]:
            written[t // s, :, int(pos[t])] = True
    for codes, scales, c16 in ((kc, ks, kc16), (vc, vs, vc16)):
        wc, wsc = K8.quant_rows_op(c16)
        assert torch.equal(codes[written], wc[written]) and torch.equal(_i32(scales[written]), _i32(wsc[written]))
        assert bool((codes[~written] == 77).all()) and bool((scales[~written] == SENT).all())  # nothing else was written


# ---- decode_attention_kv8

def _errors(o, ref, v64, pos):
    """(worst relative L2 per (row, head), worst max |o - ref| / max |v dequantised| over the keys attended)"""
    b, h, d = ref.shape
    o = o.double().reshape(b, h, d)
    rel = ((o - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)).max().item()
    vmax = max(v64[bi, :, :int(pos[bi]) + 1].abs().max().item() for bi in range(b))
    return rel, (o - ref).abs().max().item() / vmax


def _check(q, cache, pos, scale, what, **kw):
    """cache = (k codes, v codes, k scales, v scales); the reference attends to code * scale in float64"""
    from qqq_amd import ops

    kc, vc, ks, vs = cache
    xq, s1, o = ops.decode_attention_kv8(q, kc, vc, ks, vs, pos, scale, return_fp16=True, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(o).all(), what
    k64, v64 = K8.dequant64(kc, ks), K8.dequant64(vc, vs)
    ref = K8.attention64(q, k64, v64, pos, scale)
    rel, mx = _errors(o, ref, v64, pos)
    print(f"{what}: decode_attention_kv8 rel L2 {rel:.2e}, max|err|/max|v| {mx:.2e} (2^-9 = {2 ** -9:.2e})")
    assert rel <= 1e-3 and mx <= 2 ** -9, (what, rel, mx)
    wq, ws = ops.dynamic_quant(o)
    assert torch.equal(xq, wq) and torch.equal(_i32(s1), _i32(ws)), what
    return o


def _gauss_cache(dev, g, b, kvh, cap, d, k_amp=None, v_amp=None):
    k = torch.randn((b, kvh, cap, d), generator=g, device=dev)
    v = torch.randn((b, kvh, cap, d), generator=g, device=dev)
    k = k if k_amp is None else k * k_amp
    v = v if v_amp is None else v * v_amp
    kc, ks = K8.quant_rows_op(k.half())
    vc, vs = K8.quant_rows_op(v.half())
    return kc, vc, ks, vs


def _positions(dev, b, kvh, cap):
    c = _chunk(dev, b, kvh, cap)
    return c, [(0, 1, c - 1), (c, c + 1, 4095), (cap - 1, 17, 2 * c + 5)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,kvh", SHAPES)
def test_decode_attention_kv8_against_float64(dev, d, h, kvh):
    b, cap = 3, 4160
    g = torch.Generator(device=dev).manual_seed(h * 7 + kvh + d)
    cache = _gauss_cache(dev, g, b, kvh, cap, d)
    q = torch.randn((b, h, 1, d), generator=g, device=dev).half()
    c, plist = _positions(dev, b, kvh, cap)
    for p in plist:
        pos = torch.tensor(p, dtype=torch.int64, device=dev)
        _check(q, cache, pos, d ** -0.5, f"d={d} h={h} kvh={kvh} chunk={c} pos={p}")


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,kvh", [(32, 8), (14, 2)])
def test_per_token_amplitudes_and_small_value_scales(dev, d, h, kvh):
    b, cap = 3, 4160
    g = torch.Generator(device=dev).manual_seed(h + kvh + d + 1)
    q = torch.randn((b, h, 1, d), generator=g, device=dev).half()
    c, plist = _positions(dev, b, kvh, cap)
    # per-token amplitudes 2^-8 ... 2^6, mixed across tokens: the K row and the V row of a token share the token's amplitude, so the
    # keys that win a peaked softmax are also the large values, and the fp16 rounding of the small probabilities stays small against
    # the output (a per-head scale on either side is wrong by up to 2^14 on most tokens)
    amp = torch.exp2(torch.randint(-8, 7, (b, kvh, cap, 1), generator=g, device=dev).float())
    mixed = _gauss_cache(dev, g, b, kvh, cap, d, amp, amp)
    assert float(mixed[2].max() / mixed[2].min()) > 2.0 ** 12 and float(mixed[3].max() / mixed[3].min()) > 2.0 ** 12
    # every value row at 2^-8: a per-head value scale, or one folded into an fp16 probability, does not survive this
    small = _gauss_cache(dev, g, b, kvh, cap, d, None, 2.0 ** -8)
    assert float(small[3].max()) < 2.0 ** -12
    for p in plist:
        pos = torch.tensor(p, dtype=torch.int64, device=dev)
        _check(q, mixed, pos, d ** -0.5, f"mixed amplitudes d={d} h={h} kvh={kvh} pos={p}")
        _check(q, small, pos, d ** -0.5, f"values at 2^-8 d={d} h={h} kvh={kvh} pos={p}")


@pytest.mark.parametrize("d", [64, 128])
def test_peaked_softmax_and_maximum_in_the_last_split(dev, d):
    h, kvh, b, cap = 32, 8, 2, 4096
    g = torch.Generator(device=dev).manual_seed(5 + d)
    k = torch.randn((b, kvh, cap, d), generator=g, device=dev).half()
    v = torch.randn((b, kvh, cap, d), generator=g, device=dev).half()
    q = torch.randn((b, h, 1, d), generator=g, device=dev).half()
    pos = torch.tensor([cap - 1, 3000], dtype=torch.int64, device=dev)
    for bi in range(b):  # the row's last key (in its last split) aligned with every query of its KV head: a near one-hot softmax
        p = int(pos[bi])
        for kh in range(kvh):
            qs = q[bi, kh * (h // kvh):(kh + 1) * (h // kvh), 0].float().sum(0)
            k[bi, kh, p] = (qs / qs.norm() * 3 * math.sqrt(d)).half()
    kc, ks = K8.quant_rows_op(k)
    vc, vs = K8.quant_rows_op(v)
    cache = (kc, vc, ks, vs)
    _check(q, cache, pos, d ** -0.5, f"peaked d={d}")
    _check(q, cache, pos, 30 * d ** -0.5, f"scores x30 d={d}")
    q2 = (q.float() * 30).half()
    _check(q2, cache, torch.tensor([cap - 1, 1], dtype=torch.int64, device=dev), d ** -0.5, f"q x30 d={d}")


@pytest.mark.parametrize("cap", [512, 509])  # 509: head rows of scales that are not 16-byte aligned
def test_out_of_range_rows_and_the_cache_are_untouched(dev, cap):
    from qqq_amd import _lib, ops

    h, kvh, d, b, max_len = 32, 8, 128, 4, 300
    g = torch.Generator(device=dev).manual_seed(cap)
    kc, vc, ks, vs = _gauss_cache(dev, g, b, kvh, cap, d)
    # slots past max_len hold what an unwritten cache may hold: they must not reach the result of row 1
    ks[:, :, max_len:] = float("nan")
    vs[:, :, max_len:] = float("inf")
    saved = [t.clone() for t in (kc, vc, ks, vs)]
    q = torch.randn((b, h, 1, d), generator=g, device=dev).half()
    pos = torch.tensor([-1, 299, 300, cap], dtype=torch.int64, device=dev)  # only row 1 is in [0, min(cap, max_len))
    o = torch.full((b, h * d), SENT, dtype=torch.float16, device=dev)
    xq = torch.full((b, h * d), 77, dtype=torch.int8, device=dev)
    s1 = torch.full((b, 1), SENT, dtype=torch.float32, device=dev)
    L = _lib.lib()
    nb = L.qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len)
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    err = L.qqq_decode_attn_kv8(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), ks.data_ptr(), vs.data_ptr(), pos.data_ptr(), d ** -0.5,
                                o.data_ptr(), xq.data_ptr(), s1.data_ptr(), ws.data_ptr(), nb, b, h, kvh, d, cap, max_len, 0,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert err == 0, _lib.last_error()
    for bi in (0, 2, 3):
        assert bool((o[bi] == SENT).all()) and bool((xq[bi] == 77).all()) and float(s1[bi]) == SENT, bi
    for t, t0 in zip((kc, vc), saved[:2]):
        assert torch.equal(t, t0)
    for t, t0 in zip((ks, vs), saved[2:]):
        assert torch.equal(_i32(t), _i32(t0))
    ow = _check(q[1:2], tuple(t[1:2, :, :max_len].contiguous() for t in (kc, vc, ks, vs)), pos[1:2], d ** -0.5, f"row 1 cap={cap}")
    assert torch.equal(_bits(o[1:2]), _bits(ow))
    xw, sw = ops.dynamic_quant(ow)
    assert torch.equal(xq[1:2], xw) and torch.equal(_i32(s1[1:2]), _i32(sw))


def test_kv8_ops_trace_under_torch_compile(dev):
    from qqq_amd import ops

    h, kvh, d, b, cap = 28, 4, 128, 2, 256
    g = torch.Generator(device=dev).manual_seed(9)
    cos, sin = _tables(dev, cap, d, seed=11)
    kc, vc, ks, vs = _gauss_cache(dev, g, b, kvh, cap, d)
    qkv = torch.randn((b, (h + 2 * kvh) * d), generator=g, device=dev).half()
    pos = torch.tensor([200, 31], dtype=torch.int64, device=dev)

    def f(qkv, kc, vc, ks, vs, pos):
        nq, nk = h * d, kvh * d
        q_out = ops.rope_qkv_kv8(qkv[:, :nq] * 1, qkv[:, nq:nq + nk], qkv[:, nq + nk:], cos, sin, pos, kc, vc, ks, vs)
        xq, s1, o = ops.decode_attention_kv8(q_out, kc, vc, ks, vs, pos, d ** -0.5, return_fp16=True)
        return q_out, xq, s1 * 2, o

    c1 = [t.clone() for t in (kc, vc, ks, vs)]
    c2 = [t.clone() for t in (kc, vc, ks, vs)]
    eager = f(qkv, *c1, pos)
    comp = torch.compile(f, fullgraph=True)(qkv, *c2, pos)
    for e, c in zip(eager, comp):
        assert torch.equal(e.view(torch.int8), c.view(torch.int8))
    for a, b_, orig in zip(c1, c2, (kc, vc, ks, vs)):
        assert torch.equal(a.view(torch.int8), b_.view(torch.int8)) and not torch.equal(a.view(torch.int8), orig.view(torch.int8))


def test_decode_attention_kv8_hipgraph_replays_at_new_positions(dev):
    from qqq_amd import ops

    h, kvh, d, b, cap = 32, 8, 128, 2, 2048
    g = torch.Generator(device=dev).manual_seed(13)
    kc, vc, ks, vs = _gauss_cache(dev, g, b, kvh, cap, d)
    q = torch.randn((b, h, 1, d), device=dev).half()
    pos = torch.tensor([5, 9], dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.decode_attention_kv8(q, kc, vc, ks, vs, pos, d ** -0.5, max_len=cap, return_fp16=True)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = ops.decode_attention_kv8(q, kc, vc, ks, vs, pos, d ** -0.5, max_len=cap, return_fp16=True)
    torch.cuda.current_stream().wait_stream(side)
    for p in ((7, 1000), (1500, 0), (cap - 1, 129)):
        pos.copy_(torch.tensor(p, device=dev))
        q.copy_(torch.randn_like(q))
        graph.replay()
        torch.cuda.synchronize()
        want = ops.decode_attention_kv8(q, kc, vc, ks, vs, pos, d ** -0.5, max_len=cap, return_fp16=True)
        for g_, w_ in zip(out, want):
            assert torch.equal(g_.view(torch.int8), w_.view(torch.int8)), p
        _check(q, (kc, vc, ks, vs), pos, d ** -0.5, f"after replay at {p}")


# ---- the module with KVCache(dtype=torch.int8)

def _kv8_reference_step(attn, xq, s1, cache16, start):
    """The attention from existing ops: project_qkv, rope_qkv into an fp16 cache, dynamic_quant of every cached head row and its fp16
    dequantisation, SDPA, dynamic_quant, o_proj.forward_int8"""
    from qqq_amd import ops

    b = cache16.batch
    m = xq.shape[0]
    s = m // b
    h, kvh, d = attn.num_heads, attn.num_key_value_heads, attn.head_dim
    cos, sin = attn.rope_tables(cache16.capacity)
    q, k, v = attn.project_qkv(xq, s1)
    pos = cache16.positions(start, s)
    kc, vc = cache16.k[attn.layer_idx], cache16.v[attn.layer_idx]
    q_out = ops.rope_qkv(q, k, v, cos, sin, pos, kc, vc)
    n = start + s
    deq = []
    for c in (kc, vc):
        codes, sc = ops.dynamic_quant(c[:, :, :n].contiguous())
        deq.append((codes.float() * sc).half())
    mask = None
    if s > 1 and start > 0:
        mask = torch.ones((s, n), dtype=torch.bool, device=xq.device).tril(diagonal=start)
    o = F.scaled_dot_product_attention(q_out, deq[0], deq[1], attn_mask=mask, is_causal=(s > 1 and start == 0), scale=attn.scaling,
                                       enable_gqa=h != kvh)
    aq, a1 = ops.dynamic_quant(o.transpose(1, 2).reshape(b, s, h * d))
    return attn.o_proj.forward_int8(aq.reshape(m, -1), a1.reshape(m, 1))


def _layer_with(layer, x, attn_fn):
    """the decoder layer with its attention half replaced by attn_fn(xq, s1)"""
    from qqq_amd import ops

    n1, n2 = layer.input_layernorm, layer.post_attention_layernorm
    x2 = x.reshape(-1, x.shape[-1])
    xq, s1 = ops.rmsnorm_quant(x2, n1.weight, n1.variance_epsilon)
    a = attn_fn(xq, s1)
    hid = x2 + a
    mq, ms = ops.rmsnorm_quant(hid, n2.weight, n2.variance_epsilon)
    return (hid + layer.mlp.forward_int8(mq, ms)).reshape(x.shape)


@pytest.mark.parametrize("fuse", [False, True])
def test_int8_cache_layer_prefill_and_decode_against_the_composition(dev, fuse):
    from qqq_amd import KVCache

    hidden, heads, kvh, inter = 1024, 8, 2, 2048
    layer = _make_layer(dev, hidden, heads, kvh, inter, 128, False, seed=61).eval()
    if fuse:  # neither switch changes what an int8 cache does
        layer.fuse_decode()
        layer.self_attn.fuse_qkv()
    attn = layer.self_attn
    b, cap, d = 2, 600, hidden // heads
    xs = torch.randn((b, 520 + 6, hidden), device=dev).half()
    c8, c16 = KVCache(1, b, kvh, d, cap, dev, dtype=torch.int8), KVCache(1, b, kvh, d, cap, dev)
    worst = 0.0
    for start, s in [(0, 520)] + [(t, 1) for t in range(520, 526)]:
        x = xs[:, start:start + s]
        got = layer(x, c8, start)
        want = _layer_with(layer, x, lambda xq, s1: _kv8_reference_step(attn, xq, s1, c16, start))
        rel = float((got.float() - want.float()).norm() / want.float().norm())
        worst = max(worst, rel)
        print(f"int8-cache layer (fuse={fuse}), {s} token(s) at {start}: relative L2 vs the composition {rel:.2e}")
        assert torch.isfinite(got).all() and rel <= 1e-2, (start, s, rel)
        # the int8 cache holds dynamic_quant of the fp16 cache's rows, bit for bit
        for c8t, s8t, c16t in ((c8.k[0], c8.k_scale[0], c16.k[0]), (c8.v[0], c8.v_scale[0], c16.v[0])):
            wc, wsc = K8.quant_rows_op(c16t[:, :, :start + s])
            assert torch.equal(c8t[:, :, :start + s], wc) and torch.equal(_i32(s8t[:, :, :start + s]), _i32(wsc))
    print(f"int8-cache layer (fuse={fuse}): worst relative L2 {worst:.2e}")


def test_prefill_in_two_chunks_leaves_the_same_cache(dev):
    from qqq_amd import KVCache

    hidden, heads, kvh, inter = 1024, 8, 2, 2048
    layer = _make_layer(dev, hidden, heads, kvh, inter, 128, False, seed=63).eval()
    b, cap, d = 2, 256, hidden // heads
    x = torch.randn((b, 200, hidden), device=dev).half()
    one, two = KVCache(1, b, kvh, d, cap, dev, dtype=torch.int8), KVCache(1, b, kvh, d, cap, dev, dtype=torch.int8)
    o1 = layer(x, one, 0)
    o2 = torch.cat([layer(x[:, :77], two, 0), layer(x[:, 77:], two, 77)], dim=1)
    assert torch.equal(one.k[0], two.k[0]) and torch.equal(one.v[0], two.v[0])
    assert torch.equal(_i32(one.k_scale[0]), _i32(two.k_scale[0])) and torch.equal(_i32(one.v_scale[0]), _i32(two.v_scale[0]))
    assert bool(one.k[0][:, :, :200].any()) and not bool(one.k[0][:, :, 200:].any())
    rel = float((o1.float() - o2.float()).norm() / o1.float().norm())
    print(f"prefill in two chunks vs one: relative L2 of the outputs {rel:.2e}")
    assert rel <= 1e-2, rel


@pytest.mark.parametrize("gqa", [False, True])
def test_int8_cache_layer_against_transformers_llama_decoder_layer(dev, gqa):
    """transformers' fp16 LlamaDecoderLayer over the whole sequence (causal) against the quantised layer with an int8 KV cache, run as a
    32-token prefill and 8 decode steps: the 5e-2 bound on the relative L2 error of the layer's update of tests/test_gpu_attn.py and
    tests/test_gpu_decode_attn.py.  The deviation from the same layer with an fp16 cache is printed beside it."""
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
    with torch.no_grad():
        out = ref(x, attention_mask=None, position_ids=pos, position_embeddings=emb(x, pos))
        want = (out[0] if isinstance(out, tuple) else out)[:, pre:]
        runs = {}
        for dtype in (torch.int8, torch.float16):
            cache = KVCache(1, b, kvh, d, 64, dev, dtype=dtype)
            layer(x[:, :pre], cache, 0)
            runs[dtype] = torch.cat([layer(x[:, t:t + 1], cache, t) for t in range(pre, s)], dim=1)
    got = runs[torch.int8]
    du, dw = (got.float() - x[:, pre:].float()), (want.float() - x[:, pre:].float())
    rel = float((du - dw).norm() / dw.norm())
    d16 = runs[torch.float16].float() - x[:, pre:].float()
    rel16 = float((d16 - dw).norm() / dw.norm())
    dev16 = float((du - d16).norm() / d16.norm())
    print(f"int8 cache vs transformers LlamaDecoderLayer (gqa={gqa}): relative L2 error of the decode steps' update {rel:.2e} "
          f"(fp16 cache {rel16:.2e}); int8-cache update vs fp16-cache update {dev16:.2e}")
    assert torch.isfinite(got).all() and rel <= 5e-2, rel
