"""The quantiser for mixture-of-experts models on the GPU: gptq_quantize_experts against gptq_quantize per expert (an expert without
calibration rows under H = I), and quantize_model on the two-layer Qwen3-MoE and Mixtral configs of tests/test_gpu_moe.py -- every expert
linear in `results`, its codes in the stacked buffers, the rows every expert saw, a strict reload that generates the same tokens -- and
GPTQ against round-to-nearest on the final hidden state."""
import pytest
import torch
from test_gpu_moe import _config

pytestmark = pytest.mark.gpu

GS, EXPERTS, TOP_K = 128, 8, 2
NAMES = ("gate_proj", "up_proj", "down_proj")


@pytest.mark.parametrize("gs", [-1, 128])
def test_experts_are_quantised_one_by_one_and_an_unseen_one_under_the_identity(dev, gs):
    from qqq_amd.quant import gptq_quantize, gptq_quantize_experts

    g = torch.Generator().manual_seed(gs + 200)
    W = (torch.randn(3, 128, 256, generator=g) / 16).half().to(dev)
    x = torch.randn(3, 300, 256, generator=g).to(dev)
    H = 2 / 300 * x.transpose(1, 2) @ x
    H[1] = 0
    count, fallback = torch.tensor([300, 0, 300], device=dev), []
    got = gptq_quantize_experts(W, H, count, gs, fallback=fallback)
    assert fallback == [1] and len(got) == 3
    for e, res in enumerate(got):
        want = gptq_quantize(W[e], torch.eye(256, device=dev) if e == 1 else H[e], gs)
        assert torch.equal(res.weight, want.weight) and torch.equal(res.scales, want.scales) and res.grouped == (gs == 128)


def make_state_dict(cfg, seed=31):
    """a random fp16 Hugging Face state dict of `cfg` (Mixtral under its own names) and 16 x 128 calibration token ids"""
    g = torch.Generator().manual_seed(seed)
    h, v, kv, mixtral = cfg.hidden_size, cfg.vocab_size, cfg.num_key_value_heads * cfg.head_dim, cfg.model_type == "mixtral"
    rand = lambda n, k: (torch.randn((n, k), generator=g) * k ** -0.5).half()
    norm = lambda n: (1 + 0.1 * torch.randn(n, generator=g)).half()
    sd = {"model.embed_tokens.weight": torch.randn((v, h), generator=g).half(), "model.norm.weight": norm(h),
          "lm_head.weight": (0.2 * torch.randn((v, h), generator=g)).half()}
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        for name, n in (("q_proj", h), ("k_proj", kv), ("v_proj", kv), ("o_proj", h)):
            sd[f"{p}self_attn.{name}.weight"] = rand(n, h)
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = norm(h), norm(h)
        if not mixtral:
            sd[p + "self_attn.q_norm.weight"], sd[p + "self_attn.k_norm.weight"] = norm(cfg.head_dim), norm(cfg.head_dim)
        if not mixtral and i in cfg.mlp_only_layers:
            for name, (n, k) in zip(NAMES, ((cfg.intermediate_size, h), (cfg.intermediate_size, h), (h, cfg.intermediate_size))):
                sd[f"{p}mlp.{name}.weight"] = rand(n, k)
            continue
        moe, names = (p + "block_sparse_moe.", ("w1", "w3", "w2")) if mixtral else (p + "mlp.", NAMES)
        sd[moe + "gate.weight"] = torch.randn((EXPERTS, h), generator=g).half()
        for e in range(EXPERTS):
            for name, (n, k) in zip(names, ((128, h), (128, h), (h, 128))):
                sd[f"{moe}experts.{e}.{name}.weight"] = rand(n, k)
    return sd, torch.randint(0, v, (16, 128), generator=g)


def float_hidden(cfg, sd, ids, dev, replace=None):
    """the final normed hidden state of the fp16 float model on `ids`, with some linears' weights replaced"""
    from qqq_amd.quant import FloatDecoderLayer
    from qqq_amd.quant.model import _qwen3_moe_keys, _rms_norm

    sd = dict(_qwen3_moe_keys(sd), **{k + ".weight": v for k, v in (replace or {}).items()})
    x = torch.nn.functional.embedding(ids.to(dev), sd["model.embed_tokens.weight"].to(dev))
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        layer = FloatDecoderLayer(cfg, {k[len(p):]: v.to(dev) for k, v in sd.items() if k.startswith(p)})
        x = torch.cat([layer.forward(x[j:j + 1]) for j in range(x.shape[0])], dim=0)
    return _rms_norm(x, sd["model.norm.weight"].to(dev), cfg.rms_norm_eps).float()


@pytest.mark.parametrize("model_type", ["qwen3_moe", "mixtral"])
def test_quantize_model_packs_every_expert_and_gptq_beats_round_to_nearest(dev, model_type):
    """Relative L2 error of the final normed hidden state of the float layers carrying the quantised weights, against the fp16 float
    model on the calibration tokens: GPTQ's must not exceed that of round-to-nearest under the same scales.
    Measured on an MI355X, GPTQ against round-to-nearest: qwen3_moe 0.1778 against 0.2047 (0.869), mixtral 0.2009 against 0.2332 (0.861)"""
    from qqq_amd import QuantLlamaForCausalLM, pack
    from qqq_amd.quant import quantize_model, round_to_nearest
    from qqq_amd.quant.model import _qwen3_moe_keys

    cfg = _config(model_type)
    sd, ids = make_state_dict(cfg)
    results = {}
    lm = quantize_model(sd, cfg, ids, GS, device=dev, results=results, hessian="fused")
    sparse = [i for i in range(2) if model_type == "mixtral" or i not in cfg.mlp_only_layers]
    experts = {f"model.layers.{i}.mlp.experts.{e}.{n}" for i in sparse for e in range(EXPERTS) for n in NAMES}
    assert experts <= set(results) and all(f"model.layers.{i}.mlp.gate_proj" in results for i in range(2) if i not in sparse)
    for i in sparse:
        stats, ex = results[f"model.layers.{i}.mlp.experts"], lm.model.layers[i].mlp.experts
        assert int(stats["gate_up"].sum()) == int(stats["down"].sum()) == ids.numel() * TOP_K and stats["fallback"] == []
        for e in range(EXPERTS):
            res = [results[f"model.layers.{i}.mlp.experts.{e}.{n}"] for n in NAMES]
            gate_up = pack.unpack_codes(ex.gate_up_proj.B[e], True).t().to(torch.int8)
            assert torch.equal(gate_up, torch.cat([res[0].codes(), res[1].codes()])), (i, e)
            assert torch.equal(pack.unpack_codes(ex.down_proj.B[e], False).t().to(torch.int8), res[2].codes()), (i, e)  # (K = 128: per-channel)
        assert torch.equal(lm.model.layers[i].mlp.gate.weight.cpu(), _qwen3_moe_keys(sd)[f"model.layers.{i}.mlp.gate.weight"])
    fresh = QuantLlamaForCausalLM.from_config(cfg, GS)
    fresh.load_state_dict({k: v.cpu() for k, v in lm.state_dict().items()}, strict=True)
    prompts = [ids[0, :5].tolist(), ids[1, :17].tolist()]
    assert fresh.to(dev).eval().generate(prompts, 4) == lm.generate(prompts, 4)
    with pytest.raises(NotImplementedError, match="mixture-of-experts"):
        quantize_model(sd, cfg, ids, GS, device=dev, rotation="hadamard")
    linears = {k: r for k, r in results.items() if not k.endswith("mlp.experts")}
    float_w = _qwen3_moe_keys(sd)
    want = float_hidden(cfg, sd, ids, dev)
    rel = lambda got: float((got - want).norm() / want.norm())
    e_gptq = rel(float_hidden(cfg, sd, ids, dev, {k: r.weight for k, r in linears.items()}))
    e_rtn = rel(float_hidden(cfg, sd, ids, dev, {k: round_to_nearest(float_w[k + ".weight"].to(dev), r.scales, r.grouped).weight
                                                  for k, r in linears.items()}))
    print(f"{model_type}: relative L2 error of the final hidden state: GPTQ {e_gptq:.4e}, round-to-nearest {e_rtn:.4e}, ratio {e_gptq / e_rtn:.3f}")
    assert e_gptq <= e_rtn
