"""Qwen3 on the GPU: a 2-layer model (hidden 256, 4 heads, 2 KV heads, vocabulary 1000) with head_dim 128 -- not hidden / heads -- and a
second one with head_dim 64, random fp16 weights and random q_norm / k_norm weights.  The quantiser's float layer against transformers'
Qwen3DecoderLayer; quantize_model's checkpoint loads strictly, generates and keeps its norms' bits; GPTQ beats round-to-nearest on the
final hidden state; greedy tokens agree between the host path, DecodeLoop and SpecDecodeLoop over fp16 and int8 pools; rotation carries
the per-head norms through bit-identical and leaves the function alone; and the norms are no silent no-op in the attention module."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

LAYERS, HIDDEN, HEADS, KVH, INTER, VOCAB, EPS = 2, 256, 4, 2, 512, 1000, 1e-6
LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
HEAD_NORMS = ("self_attn.q_norm.weight", "self_attn.k_norm.weight")


def _config(d, **over):
    c = dict(model_type="qwen3", vocab_size=VOCAB, hidden_size=HIDDEN, num_attention_heads=HEADS, num_key_value_heads=KVH, head_dim=d,
             intermediate_size=INTER, num_hidden_layers=LAYERS, rms_norm_eps=EPS, rope_theta=10000.0, attention_bias=False,
             use_sliding_window=False, layer_types=["full_attention"] * LAYERS, tie_word_embeddings=False)
    c.update(over)
    return SimpleNamespace(**c)


def make_state_dict(d, seed=31, embed_scale=1.0):
    """a random fp16 Hugging Face Qwen3 state dict with head_dim d, and 16 x 128 calibration token ids"""
    g = torch.Generator().manual_seed(seed + d)
    h, inter, v = HIDDEN, INTER, VOCAB
    sd = {"model.embed_tokens.weight": (embed_scale * torch.randn((v, h), generator=g)).half(), "model.norm.weight": (1 + 0.1 * torch.randn(h, generator=g)).half(),
          "lm_head.weight": (0.2 * torch.randn((v, h), generator=g)).half()}
    shapes = {"self_attn.q_proj": (HEADS * d, h), "self_attn.k_proj": (KVH * d, h), "self_attn.v_proj": (KVH * d, h),
              "self_attn.o_proj": (h, HEADS * d), "mlp.gate_proj": (inter, h), "mlp.up_proj": (inter, h), "mlp.down_proj": (h, inter)}
    for i in range(LAYERS):
        for name, (n, k) in shapes.items():
            sd[f"model.layers.{i}.{name}.weight"] = (torch.randn((n, k), generator=g) * k ** -0.5).half()
        for name in ("input_layernorm", "post_attention_layernorm"):
            sd[f"model.layers.{i}.{name}.weight"] = (1 + 0.1 * torch.randn(h, generator=g)).half()
        for name in HEAD_NORMS:
            sd[f"model.layers.{i}.{name}"] = (1 + 0.3 * torch.randn(d, generator=g)).half()
    return sd, torch.randint(0, v, (16, 128), generator=g)


def float_hidden(sd, cfg, ids, dev, replace=None):
    """the final normed hidden state of the fp16 float model on `ids`, with some linears' weights replaced"""
    from qqq_amd.quant import FloatDecoderLayer
    from qqq_amd.quant.model import _rms_norm

    x = torch.nn.functional.embedding(ids.to(dev), sd["model.embed_tokens.weight"].to(dev))
    for i in range(LAYERS):
        prefix = f"model.layers.{i}."
        w = {k[len(prefix):]: v.to(dev) for k, v in sd.items() if k.startswith(prefix)}
        for k, v in (replace or {}).items():
            if k.startswith(prefix):
                w[k[len(prefix):] + ".weight"] = v.to(dev)
        layer = FloatDecoderLayer(cfg, w)
        x = torch.cat([layer.forward(x[j:j + 1]) for j in range(x.shape[0])], dim=0)
    return _rms_norm(x, sd["model.norm.weight"].to(dev), EPS)


_quantised = {}


def quantised(dev, d, gs, embed_scale=1.0):
    """(state dict, calibration ids, packed model, results) of quantize_model, once per (head_dim, group size, embedding scale)"""
    from qqq_amd.quant import quantize_model

    if (d, gs, embed_scale) not in _quantised:
        sd, ids = make_state_dict(d, embed_scale=embed_scale)
        results = {}
        _quantised[d, gs, embed_scale] = (sd, ids, quantize_model(sd, _config(d), ids, gs, device=dev, results=results), results)
    return _quantised[d, gs, embed_scale]


@pytest.mark.parametrize("d", [128, 64])
def test_float_layer_is_transformers_qwen3_decoder_layer(dev, d):
    """the bound of test_float_layer_is_transformers_decoder_layer (tests/test_gpu_gptq_model.py)"""
    tr = pytest.importorskip("transformers")
    from transformers.models.qwen3 import modeling_qwen3 as mq

    from qqq_amd.quant import FloatDecoderLayer

    sd, ids = make_state_dict(d)
    cfg = tr.Qwen3Config(vocab_size=VOCAB, hidden_size=HIDDEN, num_attention_heads=HEADS, num_key_value_heads=KVH, head_dim=d,
                         intermediate_size=INTER, num_hidden_layers=LAYERS, rms_norm_eps=EPS, max_position_embeddings=4096,
                         rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
    cfg._attn_implementation = "sdpa"
    ref = mq.Qwen3Model(cfg).to(dev).half().eval()
    with torch.no_grad():
        ref.load_state_dict({k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}, strict=True)
        x = ref.embed_tokens(ids[:2, :33].to(dev))
        pos = torch.arange(33, device=dev)[None]
        rope = ref.rotary_emb(x, pos)
        for i in range(LAYERS):
            prefix = f"model.layers.{i}."
            w = {k[len(prefix):]: v.to(dev) for k, v in sd.items() if k.startswith(prefix)}
            mine = FloatDecoderLayer(_config(d), w)
            want = ref.layers[i](x, attention_mask=None, position_ids=pos, position_embeddings=rope, use_cache=False)
            want = want[0] if isinstance(want, tuple) else want
            got = mine.forward(x)
            rel = float((got.float() - want.float()).norm() / want.float().norm())
            skipped = FloatDecoderLayer(_config(d), {k: v for k, v in w.items() if k not in HEAD_NORMS}).forward(x)
            rel_skipped = float((skipped.float() - want.float()).norm() / want.float().norm())
            print(f"head_dim {d} layer {i}: relative L2 error against transformers' Qwen3DecoderLayer {rel:.2e} (without the norms {rel_skipped:.2e})")
            assert rel <= 5e-2
            assert rel_skipped > rel  # leaving the norms out is further from transformers than any rounding
            x = want


@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("d", [128, 64])
def test_checkpoint_loads_strictly_generates_and_keeps_its_norms(dev, d, gs):
    from qqq_amd import QuantLlamaForCausalLM

    sd, ids, lm, results = quantised(dev, d, gs)
    assert sorted(results) == sorted(f"model.layers.{i}.{n}" for i in range(LAYERS) for n in LINEARS)
    fresh = QuantLlamaForCausalLM.from_config(_config(d), gs)
    fresh.load_state_dict({k: v.cpu() for k, v in lm.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    assert fresh.model.layers[0].self_attn.head_dim == d and fresh.model.layers[0].self_attn.qk_norm
    prompts = [ids[0, :5].tolist(), ids[1, :17].tolist()]
    toks = fresh.generate(prompts, 4)
    assert toks == lm.generate(prompts, 4) and all(len(t) == 4 and all(0 <= x < VOCAB for x in t) for t in toks)
    mine = fresh.state_dict()
    keys = ["model.embed_tokens.weight", "model.norm.weight", "lm_head.weight", "model.layers.1.input_layernorm.weight"]
    keys += [f"model.layers.{i}.{n}" for i in range(LAYERS) for n in HEAD_NORMS]
    for k in keys:
        assert mine[k].dtype == torch.float16 and torch.equal(mine[k].cpu().view(torch.int16), sd[k].view(torch.int16)), k


@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("d", [128, 64])
def test_gptq_beats_round_to_nearest_on_the_final_hidden_state(dev, d, gs):
    """the assertion of tests/test_gpu_gptq_model.py's test of the same name, on the Qwen3 model: no new number"""
    from qqq_amd import KVCache, QuantLlamaForCausalLM
    from qqq_amd.quant import round_to_nearest

    sd, ids, lm, results = quantised(dev, d, gs)
    cfg = _config(d)
    rtn = QuantLlamaForCausalLM.from_config(cfg, gs).to(dev)
    rtn.load_state_dict(lm.state_dict(), strict=True)
    mods = dict(rtn.named_modules())
    rtn_w = {}
    for name, res in results.items():
        r = round_to_nearest(sd[name + ".weight"].to(dev), res.scales, gs != -1)
        r.pack_into(mods[name])
        rtn_w[name] = r.weight

    def quant_hidden(m):
        with torch.no_grad():
            return m.model(ids.to(dev), KVCache(LAYERS, ids.shape[0], KVH, d, ids.shape[1], dev), 0, all_rows=True)

    want = float_hidden(sd, cfg, ids, dev).float()
    rel = lambda got: float((got.float().reshape(want.shape) - want).norm() / want.norm())
    e_gptq, e_rtn = rel(quant_hidden(lm)), rel(quant_hidden(rtn.eval()))
    w_gptq = rel(float_hidden(sd, cfg, ids, dev, {n: r.weight for n, r in results.items()}))
    w_rtn = rel(float_hidden(sd, cfg, ids, dev, rtn_w))
    print(f"head_dim {d} gs {gs}: relative L2 error of the final hidden state: GPTQ {e_gptq:.4e}, round-to-nearest {e_rtn:.4e}, ratio "
          f"{e_gptq / e_rtn:.3f}; weights only (float layers): GPTQ {w_gptq:.4e}, round-to-nearest {w_rtn:.4e}, ratio {w_gptq / w_rtn:.3f}")
    assert e_gptq < e_rtn
    assert w_gptq < w_rtn


@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("d", [128, 64])
def test_greedy_tokens_agree_between_the_host_path_and_the_device_loops(dev, d, gs):
    """The three paths run different attention kernels and split plans (the host path's decode batch, the loop's max_len, the speculative
    step's chunk through the prefill kernel), so their hidden states agree to the last bits only, and a greedy token can differ where
    the two best logits are nearly tied.  The model here has its embeddings scaled by 4 against the layers' updates, as the model of
    tests/test_gpu_spec_loop.py: the last bits of an attention output then weigh a quarter as much in the final hidden state.
    Measured on an MI355X with the embeddings NOT scaled (head_dim 128, per-channel, int8 pool): the speculative loop left the host path
    at one token whose two best logits were 8.4453 and 8.4375, one fp16 ulp apart; every other decision of that run had a margin of
    0.09 ... 1.0.  With the scaling all sixteen (head_dim, group size, pool, path) combinations agree."""
    sd, ids, lm, _ = quantised(dev, d, gs, embed_scale=4.0)
    prompts = [ids[0, :5].tolist(), ids[1, :17].tolist(), ids[2, :33].tolist()]
    lm.fuse_prefill()
    try:
        for dtype in (torch.float16, torch.int8):
            with torch.no_grad():
                host = lm.generate(prompts, 8, dtype=dtype)
                loop = lm.generate(prompts, 8, dtype=dtype, device_loop=True)
                spec = lm.generate(prompts, 8, dtype=dtype, device_loop=True, draft_len=3)
            print(f"head_dim {d} gs {gs} {dtype}: host {host}\n  DecodeLoop {loop}\n  SpecDecodeLoop {spec}")
            assert all(len(t) == 8 and all(0 <= x < VOCAB for x in t) for t in host)
            assert loop == host, (d, gs, dtype)
            assert spec == host, (d, gs, dtype)
    finally:
        lm.model.unfuse_prefill()


@pytest.mark.parametrize("d", [128, 64])
def test_rotation_carries_the_head_norms_through_and_leaves_the_function_alone(dev, d):
    """q_norm / k_norm come back bit-identical, from rotate_model and in quantize_model(rotation="hadamard")'s packed model.  The float
    function: fp32 logits of the rotated weights on the GPU against an fp64 forward of the unrotated ones, relative L2 deviation below
    1e-2 -- the ceiling tests/test_gpu_rotate_k.py's test_rotation_leaves_the_models_function_alone holds the reference's rotated
    weights to (fp16 rounding of every weight, twice) -- and far above the fp32 forward's own."""
    from qqq_amd.quant import FloatDecoderLayer, quantize_model, rotate_model
    from qqq_amd.quant.model import _rms_norm

    sd, ids = make_state_dict(d)
    cfg = _config(d)
    rotated, signs = rotate_model(sd, cfg, generator=torch.Generator().manual_seed(5), device=dev)
    norms = [f"model.layers.{i}.{n}" for i in range(LAYERS) for n in HEAD_NORMS]
    for k in norms:
        assert torch.equal(rotated[k].view(torch.int16), sd[k].view(torch.int16)), k
    assert all(bool((rotated[f"model.layers.{i}.input_layernorm.weight"] == 1).all()) for i in range(LAYERS))
    assert not torch.equal(rotated["model.layers.0.self_attn.q_proj.weight"], sd["model.layers.0.self_attn.q_proj.weight"])

    def logits(state, dtype, where):
        t = {k: v.to(where).to(dtype) for k, v in state.items()}
        x = torch.nn.functional.embedding(ids[:2, :16].to(where), t["model.embed_tokens.weight"])
        for i in range(LAYERS):
            p = f"model.layers.{i}."
            x = FloatDecoderLayer(cfg, {k[len(p):]: v for k, v in t.items() if k.startswith(p)}).forward(x)
        return (_rms_norm(x, t["model.norm.weight"], EPS) @ t["lm_head.weight"].t()).double().cpu()

    want = logits(sd, torch.float64, "cpu")
    rel = lambda a: float((a - want).norm() / want.norm())
    plain, mine = rel(logits(sd, torch.float32, dev)), rel(logits(rotated, torch.float32, dev))
    broken = dict(rotated)
    broken["model.layers.0.self_attn.q_norm.weight"] = torch.ones_like(sd["model.layers.0.self_attn.q_norm.weight"])
    lost = rel(logits(broken, torch.float32, dev))
    print(f"head_dim {d}: relative L2 deviation of the logits: fp32 forward alone {plain:.3e}, rotated weights {mine:.3e}, one q_norm lost {lost:.3e}")
    assert plain < mine / 20 and 0 < mine < 1e-2
    assert lost > 2 * mine  # a folded-away or reset head norm is another function, not rounding

    results = {}
    lm = quantize_model(sd, cfg, ids[:4], 128, mse=True, device=dev, results=results, rotation=signs)
    assert torch.equal(results["rotation"], signs)
    mine_sd = lm.state_dict()
    for k in norms:
        assert torch.equal(mine_sd[k].cpu().view(torch.int16), sd[k].view(torch.int16)), k
    toks = lm.generate([ids[0, :5].tolist()], 4)
    assert len(toks[0]) == 4


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_the_norms_are_no_silent_no_op_in_the_attention_module(dev, dtype):
    from qqq_amd import KVCache

    sd, ids, lm, _ = quantised(dev, 128, 128)
    attn = lm.model.layers[0].self_attn
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn((1, 9, HIDDEN), generator=g, device=dev).half()

    def run():
        with torch.no_grad():
            return attn(x, KVCache(LAYERS, 1, KVH, 128, 16, dev, dtype=dtype), 0)

    with_norms = run()
    again = run()
    attn.qk_norm = False
    try:
        skipped = run()
    finally:
        attn.qk_norm = True
    assert torch.equal(with_norms, again)
    rel = float((with_norms.float() - skipped.float()).norm() / skipped.float().norm())
    print(f"{dtype}: relative L2 difference of the attention output with and without the norms {rel:.3e}")
    assert rel > 1e-2
