"""quantize_model on the GPU over the 2-layer model of tests/test_gpu_model.py (256 / 4 / 2 / 512, vocabulary 1000) with random fp16
weights, calibrated on 16 x 128 random tokens: the checkpoint loads strictly and generates, every packed layer holds its result's codes,
GPTQ beats round-to-nearest under the same scales on the final hidden state, the command-line tool round-trips, and the float layer the
flow runs on is transformers' decoder layer."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = dict(model_type="llama", vocab_size=1000, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
              num_hidden_layers=2, rms_norm_eps=1e-6, rope_theta=10000.0)
LAYERS, KVH, D = 2, 2, 64
SEED = 21
LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def make_state_dict(seed=SEED):
    """a random fp16 Hugging Face state dict of CONFIG, and 16 x 128 calibration token ids"""
    g = torch.Generator().manual_seed(seed)
    h, inter, v, kv = CONFIG["hidden_size"], CONFIG["intermediate_size"], CONFIG["vocab_size"], KVH * D
    sd = {"model.embed_tokens.weight": torch.randn((v, h), generator=g).half(), "model.norm.weight": (1 + 0.1 * torch.randn(h, generator=g)).half(),
          "lm_head.weight": (0.2 * torch.randn((v, h), generator=g)).half()}
    shapes = {"self_attn.q_proj": (h, h), "self_attn.k_proj": (kv, h), "self_attn.v_proj": (kv, h), "self_attn.o_proj": (h, h),
              "mlp.gate_proj": (inter, h), "mlp.up_proj": (inter, h), "mlp.down_proj": (h, inter)}
    for i in range(LAYERS):
        for name, (n, k) in shapes.items():
            sd[f"model.layers.{i}.{name}.weight"] = (torch.randn((n, k), generator=g) * k ** -0.5).half()
        for name in ("input_layernorm", "post_attention_layernorm"):
            sd[f"model.layers.{i}.{name}.weight"] = (1 + 0.1 * torch.randn(h, generator=g)).half()
    ids = torch.randint(0, v, (16, 128), generator=g)
    return sd, ids


def float_hidden(sd, ids, dev, replace=None):
    """the final normed hidden state of the fp16 float model on `ids`, with some linears' weights replaced"""
    from qqq_amd.quant import FloatDecoderLayer
    from qqq_amd.quant.model import _rms_norm

    cfg = SimpleNamespace(**CONFIG)
    x = torch.nn.functional.embedding(ids.to(dev), sd["model.embed_tokens.weight"].to(dev))
    for i in range(LAYERS):
        prefix = f"model.layers.{i}."
        w = {k[len(prefix):]: v.to(dev) for k, v in sd.items() if k.startswith(prefix)}
        for k, v in (replace or {}).items():
            if k.startswith(prefix):
                w[k[len(prefix):] + ".weight"] = v.to(dev)
        layer = FloatDecoderLayer(cfg, w)
        x = torch.cat([layer.forward(x[j:j + 1]) for j in range(x.shape[0])], dim=0)
    return _rms_norm(x, sd["model.norm.weight"].to(dev), CONFIG["rms_norm_eps"])


@pytest.fixture(scope="module")
def quantised(dev):
    from qqq_amd.quant import quantize_model

    sd, ids = make_state_dict()
    out = {}
    for gs in (-1, 128):
        results = {}
        out[gs] = (quantize_model(sd, SimpleNamespace(**CONFIG), ids, gs, device=dev, results=results), results)
    return sd, ids, out


def _quant_hidden(lm, ids, dev):
    from qqq_amd import KVCache

    with torch.no_grad():
        return lm.model(ids.to(dev), KVCache(LAYERS, ids.shape[0], KVH, D, ids.shape[1], dev), 0, all_rows=True)


@pytest.mark.parametrize("gs", [-1, 128])
def test_checkpoint_loads_strictly_generates_and_holds_its_codes(dev, quantised, gs):
    from qqq_amd import QuantLlamaForCausalLM, pack

    sd, ids, out = quantised
    lm, results = out[gs]
    assert sorted(results) == sorted(f"model.layers.{i}.{n}" for i in range(LAYERS) for n in LINEARS)
    fresh = QuantLlamaForCausalLM.from_config(SimpleNamespace(**CONFIG), gs)
    fresh.load_state_dict({k: v.cpu() for k, v in lm.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    prompts = [ids[0, :5].tolist(), ids[1, :17].tolist()]
    toks = fresh.generate(prompts, 4)
    assert toks == lm.generate(prompts, 4) and all(len(t) == 4 and all(0 <= x < CONFIG["vocab_size"] for x in t) for t in toks)
    mods = dict(fresh.named_modules())
    for name, res in results.items():
        codes = pack.unpack_codes(mods[name].B, gs != -1).t().to(torch.int8)
        assert torch.equal(codes, res.codes()), name
        lo, hi = (0, 15) if gs != -1 else (-7, 7)
        assert int(codes.min()) >= lo and int(codes.max()) <= hi and codes.float().std() > 1
    for k in ("model.embed_tokens.weight", "model.norm.weight", "lm_head.weight", "model.layers.1.input_layernorm.weight"):
        assert torch.equal(fresh.state_dict()[k].cpu(), sd[k]), k


@pytest.mark.parametrize("gs", [-1, 128])
def test_gptq_beats_round_to_nearest_on_the_final_hidden_state(dev, quantised, gs):
    """Relative L2 error of the final normed hidden state on the calibration tokens against the fp16 float model: the GPTQ checkpoint's
    must be below that of the same model rounded to nearest under the same scales.  With the float layers carrying the quantised weights
    (no activation quantisation) the CPU restatement gives GPTQ / RTN = 0.879 (per-channel: 0.167 against 0.191) and 0.879 (g128: 0.143
    against 0.163) on this seed.  Measured on an MI355X, packed models with the int8 activations on top: 0.1684 against 0.1913 (0.881)
    per-channel, 0.1446 against 0.1641 (0.881) g128; float layers with the quantised weights: 0.880 and 0.879."""
    from qqq_amd import QuantLlamaForCausalLM
    from qqq_amd.quant import round_to_nearest

    sd, ids, out = quantised
    lm, results = out[gs]
    rtn = QuantLlamaForCausalLM.from_config(SimpleNamespace(**CONFIG), gs).to(dev)
    rtn.load_state_dict(lm.state_dict(), strict=True)
    mods = dict(rtn.named_modules())
    rtn_w = {}
    for name, res in results.items():
        r = round_to_nearest(sd[name + ".weight"].to(dev), res.scales, gs != -1)
        r.pack_into(mods[name])
        rtn_w[name] = r.weight
    want = float_hidden(sd, ids, dev).float()
    rel = lambda got: float((got.float().reshape(want.shape) - want).norm() / want.norm())
    e_gptq, e_rtn = rel(_quant_hidden(lm, ids, dev)), rel(_quant_hidden(rtn.eval(), ids, dev))
    w_gptq = rel(float_hidden(sd, ids, dev, {n: r.weight for n, r in results.items()}))
    w_rtn = rel(float_hidden(sd, ids, dev, rtn_w))
    print(f"gs {gs}: relative L2 error of the final hidden state: GPTQ {e_gptq:.4e}, round-to-nearest {e_rtn:.4e}, ratio {e_gptq / e_rtn:.3f}; "
          f"weights only (float layers): GPTQ {w_gptq:.4e}, round-to-nearest {w_rtn:.4e}, ratio {w_gptq / w_rtn:.3f}")
    assert e_gptq < e_rtn
    assert w_gptq < w_rtn


def test_command_line_tool_round_trips(dev, quantised, tmp_path):
    from qqq_amd import QuantLlamaForCausalLM

    sd, ids, out = quantised
    json.dump(CONFIG, open(tmp_path / "config.json", "w"))
    torch.save(sd, tmp_path / "model.pt")
    np.save(tmp_path / "calib.npy", ids.numpy())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "quantize_model.py"), "--config", str(tmp_path / "config.json"), "--weights",
                        str(tmp_path / "model.pt"), "--tokens", str(tmp_path / "calib.npy"), "--group-size", "128", "--seqlen", "128", "--out",
                        str(tmp_path / "q")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["group_size"] == 128 and line["nsamples"] == 16 and line["linears"] == 14
    assert json.load(open(tmp_path / "q" / "quant_config.json")) == {"group_size": 128, "wbits": 4}
    saved = torch.load(tmp_path / "q" / "model.pt", map_location="cpu", weights_only=True)
    mine = out[128][0].state_dict()
    assert sorted(saved) == sorted(mine)
    for k, v in saved.items():  # the same flow on the same inputs: the same checkpoint
        assert torch.equal(v, mine[k].cpu()), k
    fresh = QuantLlamaForCausalLM.from_config(SimpleNamespace(**CONFIG), 128)
    fresh.load_state_dict(saved, strict=True)


def test_float_layer_is_transformers_decoder_layer(dev):
    tr = pytest.importorskip("transformers")
    from transformers.models.llama import modeling_llama as ml

    from qqq_amd.quant import FloatDecoderLayer

    sd, ids = make_state_dict()
    cfg = tr.LlamaConfig(vocab_size=CONFIG["vocab_size"], hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
                         num_hidden_layers=LAYERS, rms_norm_eps=1e-6, max_position_embeddings=4096,
                         rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
    cfg._attn_implementation = "sdpa"
    ref = ml.LlamaModel(cfg).to(dev).half().eval()
    with torch.no_grad():
        ref.load_state_dict({k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}, strict=True)
        x = ref.embed_tokens(ids[:2, :33].to(dev))
        pos = torch.arange(33, device=dev)[None]
        rope = ref.rotary_emb(x, pos)
        for i in range(LAYERS):
            prefix = f"model.layers.{i}."
            mine = FloatDecoderLayer(SimpleNamespace(**CONFIG), {k[len(prefix):]: v.to(dev) for k, v in sd.items() if k.startswith(prefix)})
            want = ref.layers[i](x, attention_mask=None, position_ids=pos, position_embeddings=rope, use_cache=False)
            want = want[0] if isinstance(want, tuple) else want
            got = mine.forward(x)
            rel = float((got.float() - want.float()).norm() / want.float().norm())
            print(f"layer {i}: relative L2 error against transformers' LlamaDecoderLayer {rel:.2e}")
            assert rel <= 5e-2
            x = want
