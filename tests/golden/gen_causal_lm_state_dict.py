#!/usr/bin/env python3
"""Generate tests/golden/causal_lm_state_dict.json: the state-dict entry names, shapes and dtypes of the reference's
QuantizedLlamaForCausalLM and QuantizedQwen2ForCausalLM (QQQ/gptq/models/llama.py, qwen2.py) for one tiny config each.

The reference's model classes do not import under the transformers installed here (5.x: they subclass LlamaSdpaAttention and friends of
4.38, and QQQ.utils needs packages that are absent), so the entries are DERIVED BY READING the class definitions, not by instantiating
them.  What was read:
  Quantized*ForCausalLM      model, lm_head = nn.Linear(hidden, vocab, bias=False)                       -> lm_head.weight
  Quantized*Model            embed_tokens = nn.Embedding(vocab, hidden), layers, norm = *RMSNorm         -> model.embed_tokens.weight,
                             (causal_mask is registered persistent=False)                                   model.norm.weight
  Quantized*DecoderLayer     self_attn, mlp, input_layernorm, post_attention_layernorm (RMSNorm .weight)
  Quantized*Attention        q_proj, k_proj, v_proj, o_proj QuantLinears; bias = config.attention_bias for all four (Llama); True, True, True,
                             False (Qwen2); o_proj is hidden -> hidden; the rotary embedding's inv_freq is persistent=False
  Quantized*MLP              gate_proj, up_proj, down_proj QuantLinears, bias=False
  QuantLinear (qlinear_marlin.py)   persistent buffers B int32 [K / 16, N * 16 / 8], s_channel f32 [1, N], s_group f16 [K / group, N] (or an
                             empty f16 tensor for a per-channel layer), bias f16 [N] where asked for; workspace and reduce_buffer are
                             persistent=False
This file restates names and shapes; it holds no reference code.  The parameters' dtype is the fp16 the reference's loader casts to.

usage: python tests/golden/gen_causal_lm_state_dict.py      (writes tests/golden/causal_lm_state_dict.json)
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

CONFIGS = {
    "llama": dict(model_type="llama", vocab_size=1000, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
                  num_hidden_layers=2, rms_norm_eps=1e-5, attention_bias=False, tie_word_embeddings=False, hidden_act="silu",
                  rope_theta=10000.0, group_size=128),
    "qwen2": dict(model_type="qwen2", vocab_size=1000, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
                  num_hidden_layers=3, rms_norm_eps=1e-6, tie_word_embeddings=True, hidden_act="silu", rope_theta=1000000.0,
                  use_sliding_window=False, group_size=-1),
}


def quant_linear(prefix, k, n, group_size, bias):
    e = {prefix + ".B": ([k // 16, n * 16 // 8], "int32"), prefix + ".s_channel": ([1, n], "float32"),
         prefix + ".s_group": ([k // group_size, n] if group_size not in (-1, k) else [0], "float16")}
    if bias:
        e[prefix + ".bias"] = ([n], "float16")
    return e


def entries(c):
    h, heads, kvh, inter, gs = c["hidden_size"], c["num_attention_heads"], c["num_key_value_heads"], c["intermediate_size"], c["group_size"]
    d = h // heads
    qwen2 = c["model_type"] == "qwen2"
    qkv_bias = True if qwen2 else c["attention_bias"]
    o_bias = False if qwen2 else c["attention_bias"]
    e = {"model.embed_tokens.weight": ([c["vocab_size"], h], "float16")}
    for i in range(c["num_hidden_layers"]):
        p = f"model.layers.{i}."
        e.update(quant_linear(p + "self_attn.q_proj", h, heads * d, gs, qkv_bias))
        e.update(quant_linear(p + "self_attn.k_proj", h, kvh * d, gs, qkv_bias))
        e.update(quant_linear(p + "self_attn.v_proj", h, kvh * d, gs, qkv_bias))
        e.update(quant_linear(p + "self_attn.o_proj", h, h, gs, o_bias))
        e.update(quant_linear(p + "mlp.gate_proj", h, inter, gs, False))
        e.update(quant_linear(p + "mlp.up_proj", h, inter, gs, False))
        e.update(quant_linear(p + "mlp.down_proj", inter, h, gs, False))
        e[p + "input_layernorm.weight"] = ([h], "float16")
        e[p + "post_attention_layernorm.weight"] = ([h], "float16")
    e["model.norm.weight"] = ([h], "float16")
    e["lm_head.weight"] = ([c["vocab_size"], h], "float16")
    return e


if __name__ == "__main__":
    out = {name: dict(config=c, entries={k: dict(shape=s, dtype=t) for k, (s, t) in entries(c).items()}) for name, c in CONFIGS.items()}
    with open(os.path.join(HERE, "causal_lm_state_dict.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
