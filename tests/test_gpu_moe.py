"""Mixture-of-experts layers on the GPU: moe_route against an f64 softmax and numpy's stable argsort, moe_gemm at 0 ulp against the numpy
reference per expert, moe_combine against an f64 sum, QuantSparseMoeBlock against a loop over QuantLinear.forward_int8 (eager and from a
captured graph), and a two-layer Qwen3-MoE / a Mixtral model through generate() on the host path and both device loops."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import qqq_ref as R
from test_gpu_attn import _make_ql

pytestmark = pytest.mark.gpu


def _logits(T, E, seed):
    """every row a random permutation of E distinct fp16 values 1/8 apart"""
    rng = np.random.default_rng(seed)
    vals = ((np.arange(E) - E // 2) / 8).astype(np.float16)
    return np.stack([rng.permutation(vals) for _ in range(T)])


def _sorted_pairs(ids, E):
    flat = ids.reshape(-1)
    return np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=E))]), np.argsort(flat, kind="stable")


@pytest.mark.parametrize("T,E,k,renorm", [(1, 8, 2, True), (5, 128, 8, True), (130, 64, 6, False), (300, 128, 8, True)])
def test_route(dev, T, E, k, renorm):
    from qqq_amd import ops

    x = _logits(T, E, seed=T)
    xt = torch.from_numpy(x).to(dev)
    ids, w, offsets, order = (t.cpu().numpy() for t in ops.moe_route(xt, k, renorm))
    p = np.exp(x.astype(np.float64) - x.astype(np.float64).max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    want_ids = np.argsort(-p, axis=-1, kind="stable")[:, :k]
    want_w = np.take_along_axis(p, want_ids, -1)
    want_w = want_w / want_w.sum(-1, keepdims=True) if renorm else want_w
    assert np.array_equal(ids, want_ids)
    want_offsets, want_order = _sorted_pairs(ids, E)
    assert np.array_equal(offsets, want_offsets) and np.array_equal(order, want_order)
    base = torch.softmax(xt, dim=-1, dtype=torch.float32).topk(k, dim=-1).values
    base = (base / base.sum(-1, keepdim=True) if renorm else base).cpu().numpy()
    err, err_base = (float(np.abs(v.astype(np.float64) / want_w - 1).max()) for v in (w, base))
    print(f"T {T} E {E} top_k {k} renorm {renorm}: largest relative error of w {err:.3e}, of torch's f32 softmax + topk {err_base:.3e}")
    assert err <= 2 * err_base


def test_route_ties_go_to_the_lower_expert_and_bad_rows_keep_valid_ids(dev):
    from qqq_amd import ops

    E, k = 16, 3
    x = _logits(6, E, seed=9)
    tie = np.sort(x[0])[::-1].copy()          # descending: experts 0, 1, 2 would win; make experts 2 and 3 equal at the cut
    tie[3] = tie[2]
    x[0] = tie[[3, 1, 0, 2] + list(range(4, E))]  # the two equal logits now sit at experts 0 and 3, the larger two at 2 and 1
    bad = x.copy()
    bad[2, :] = np.nan
    bad[4, 5] = np.inf
    ids = ops.moe_route(torch.from_numpy(x).to(dev), k, True)[0].cpu().numpy()
    ids_bad, _, offsets, order = (t.cpu().numpy() for t in ops.moe_route(torch.from_numpy(bad).to(dev), k, True))
    assert ids[0].tolist() == [2, 1, 0]
    assert ids_bad.min() >= 0 and ids_bad.max() < E and all(len(set(r)) == k for r in ids_bad.tolist())
    keep = [0, 1, 3, 5]
    assert np.array_equal(ids_bad[keep], ids[keep])
    want_offsets, want_order = _sorted_pairs(ids_bad, E)
    assert np.array_equal(offsets, want_offsets) and np.array_equal(order, want_order)


COUNTS = (0, 1, 16, 17, 70)  # rows per expert: none, one, one tile, two tiles, a second pass with a ragged tail


@pytest.mark.parametrize("K,N", [(128, 64), (256, 192), (512, 128)])
@pytest.mark.parametrize("a_div", [1, 2])
@pytest.mark.parametrize("gs", [-1, 128])
def test_grouped_gemm_is_the_dense_gemm_per_expert(dev, gs, a_div, K, N):
    from qqq_amd import ops

    rng = np.random.default_rng(K + N + a_div)
    E, k, grouped = len(COUNTS), 2, gs != -1
    P = sum(COUNTS)
    ids = rng.permutation(np.repeat(np.arange(E), COUNTS)).astype(np.int32)
    offsets, order = _sorted_pairs(ids, E)
    codes = rng.integers(0, 16, (E, K, N), dtype=np.int8) if grouped else rng.integers(-7, 8, (E, K, N), dtype=np.int8)
    B = np.stack([R.pack_codes(c, grouped) for c in codes])
    s2 = (rng.random((E, N), dtype=np.float32) * 2e-4 + 1e-5)
    s3 = (rng.random((E, K // 128, N), dtype=np.float32) * 1.5 + 0.05).astype(np.float16) if grouped else np.zeros((0,), np.float16)
    rows = P // a_div
    xq = rng.integers(-128, 128, (rows, K), dtype=np.int8)
    s1 = (rng.random(rows, dtype=np.float32) * 0.05 + 0.001)
    want = np.zeros((P, N), np.float16)
    for e in range(E):
        pairs = order[offsets[e]:offsets[e + 1]]
        if len(pairs):
            a = pairs // a_div
            want[pairs] = R.qqq_gemm(xq[a], B[e], s1[a, None], s2[e][None], s3[e] if grouped else None)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    reverse = np.concatenate([order[offsets[e]:offsets[e + 1]][::-1] for e in range(E)])
    for od in (order, reverse):
        got = ops.moe_gemm(t(xq), t(s1), t(B), t(s2), t(s3), t(ids), t(offsets.astype(np.int32)), t(od.astype(np.int32)), k, a_div, gs)
        assert np.array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16))


@pytest.mark.parametrize("T,k,H", [(3, 1, 64), (17, 8, 2048), (5, 16, 136)])
def test_combine(dev, T, k, H):
    from qqq_amd import ops

    g = torch.Generator().manual_seed(T)
    y = torch.randn((T * k, H), generator=g).half()
    w = torch.rand((T, k), generator=g)
    got = ops.moe_combine(y.to(dev), w.to(dev), k).cpu()
    want = (w.double()[:, :, None] * y.double().reshape(T, k, H)).sum(1).half()
    ulp = torch.maximum(want.abs().float(), torch.tensor(2.0 ** -14)).log2().floor().exp2() * 2.0 ** -10
    assert bool(((got.float() - want.float()).abs() <= ulp).all())


def _block(dev, gs, seed=3, E=8, k=2, hidden=256, inter=128):
    from qqq_amd import QuantSparseMoeBlock

    blk = QuantSparseMoeBlock(hidden, inter, E, k, True, gs).to(dev)
    blk.gate.weight.data = torch.randn((E, hidden), generator=torch.Generator().manual_seed(seed)).half().to(dev)
    # (a QuantLinear whose one group spans all of K -- down_proj here -- is the per-channel format: QuantLinear's own rule)
    qls = [[_make_ql(dev, K, N, gs if K != 128 else -1, False, seed + 10 * e + i) for i, (K, N) in
            enumerate(((hidden, inter), (hidden, inter), (inter, hidden)))] for e in range(E)]
    for e, (gate, up, down) in enumerate(qls):
        blk.experts.load_expert(e, gate, up, down)
    return blk, qls


@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("T", [1, 37])
def test_block_is_the_loop_over_quant_linears_eager_and_replayed(dev, T, gs):
    import torch.nn.functional as F

    from qqq_amd import ops

    blk, qls = _block(dev, gs)
    g = torch.Generator().manual_seed(T)
    x, x2 = (torch.randn((T, 256), generator=g).half().to(dev) for _ in range(2))

    def loop(x):
        xq, s1 = ops.dynamic_quant(x)
        ids, w, _, _ = ops.moe_route(F.linear(x, blk.gate.weight), 2, True)
        acc = torch.zeros((T, 256), device=dev)
        for j in range(2):
            rows = []
            for t, e in enumerate(ids[:, j].tolist()):
                gate, up, down = qls[e]
                hq, hs = ops.silu_mul_quant(gate.forward_int8(xq[t:t + 1], s1[t:t + 1]), up.forward_int8(xq[t:t + 1], s1[t:t + 1]))
                rows.append(down.forward_int8(hq, hs))
            acc = acc + w[:, j:j + 1] * torch.cat(rows).float()
        return acc.half()

    with torch.no_grad():
        assert torch.equal(blk(x).view(torch.int16), loop(x).view(torch.int16))
        buf = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            blk(buf)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = blk(buf)
        buf.copy_(x2)
        graph.replay()
        assert torch.equal(out.view(torch.int16), blk(x2).view(torch.int16)) and not torch.equal(out, blk(x))
        buf.copy_(x)
        graph.replay()
        assert torch.equal(out.view(torch.int16), blk(x).view(torch.int16))
        with pytest.raises(NotImplementedError):
            blk.forward_int8(*ops.dynamic_quant(x), x, lora=object())


def _config(model_type, **over):
    c = dict(model_type=model_type, vocab_size=1000, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
             intermediate_size=512, num_hidden_layers=2, rms_norm_eps=1e-6, rope_theta=10000.0, attention_bias=False,
             tie_word_embeddings=False, num_experts_per_tok=2)
    if model_type == "qwen3_moe":
        c.update(num_experts=8, moe_intermediate_size=128, norm_topk_prob=True, mlp_only_layers=[0], decoder_sparse_step=1,
                 use_sliding_window=False)
    else:
        c.update(num_local_experts=8, intermediate_size=128, sliding_window=None)
    c.update(over)
    return SimpleNamespace(**c)


def _random_lm(dev, cfg, gs, seed=11):
    """the config's model with random packed weights: any int32 is a packed word, the scales as tests/test_gpu_attn.py draws them"""
    from qqq_amd import QuantLlamaForCausalLM

    lm = QuantLlamaForCausalLM.from_config(cfg, gs)
    g = torch.Generator().manual_seed(seed)
    sd = lm.state_dict()
    for name, v in sd.items():
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "B":
            v.copy_(torch.randint(-2 ** 31, 2 ** 31, v.shape, generator=g, dtype=torch.int64).int())
        elif leaf == "s_channel":
            v.copy_(torch.rand(v.shape, generator=g) * 2e-4 + 1e-5)
        elif leaf == "s_group":
            v.copy_(torch.rand(v.shape, generator=g) * 1.5 + 0.05)
        elif "norm" in name:
            v.copy_(1 + 0.1 * torch.randn(v.shape, generator=g))
        else:  # the embedding (scaled by 4 against the layers' updates, as tests/test_gpu_qwen3_model.py), lm_head and the routers
            v.copy_((4.0 if "embed" in name else 0.2 if "lm_head" in name else 1.0) * torch.randn(v.shape, generator=g))
    return lm.to(dev).eval(), sd


@pytest.mark.parametrize("gs", [-1, 128])
def test_qwen3_moe_generates_the_same_tokens_on_the_host_path_and_in_both_device_loops(dev, gs):
    from qqq_amd import QuantLlamaForCausalLM, QuantLlamaMLP, QuantSparseMoeBlock

    cfg = _config("qwen3_moe")
    lm, sd = _random_lm(dev, cfg, gs)
    kinds = [type(layer.mlp) for layer in lm.model.layers]
    assert kinds == [QuantLlamaMLP, QuantSparseMoeBlock]
    assert {"model.layers.1.mlp.gate.weight", "model.layers.1.mlp.experts.gate_up_proj.B", "model.layers.1.mlp.experts.gate_up_proj.s_channel",
            "model.layers.1.mlp.experts.gate_up_proj.s_group", "model.layers.1.mlp.experts.down_proj.B",
            "model.layers.1.mlp.experts.down_proj.s_channel", "model.layers.1.mlp.experts.down_proj.s_group"} <= set(sd)
    fresh = QuantLlamaForCausalLM.from_config(cfg, gs)
    fresh.load_state_dict({k: v.cpu() for k, v in lm.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, 1000, (n,), generator=g).tolist() for n in (5, 17)]
    lm.fuse_prefill()
    with torch.no_grad():
        host = lm.generate(prompts, 8, temperature=0)
        assert all(len(t) == 8 for t in host) and fresh.generate(prompts, 8, temperature=0) == host
        assert lm.generate(prompts, 8, temperature=0, device_loop=True) == host
        assert lm.generate(prompts, 8, temperature=0, device_loop=True, draft_len=2) == host


def test_mixtral_builds_and_runs_and_refuses_a_sliding_window(dev):
    from qqq_amd import KVCache, QuantLlamaForCausalLM, QuantSparseMoeBlock

    lm, _ = _random_lm(dev, _config("mixtral"), 128)
    assert all(isinstance(layer.mlp, QuantSparseMoeBlock) and layer.mlp.norm_topk_prob for layer in lm.model.layers)
    ids = torch.randint(0, 1000, (2, 9), generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        logits = lm(ids, KVCache(2, 2, 2, 64, 16, dev), 0)
    assert logits.shape == (2, 1000) and bool(torch.isfinite(logits.float()).all())
    with pytest.raises(NotImplementedError):
        QuantLlamaForCausalLM.from_config(_config("mixtral", sliding_window=4096), 128)
