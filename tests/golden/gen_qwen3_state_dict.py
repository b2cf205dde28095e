#!/usr/bin/env python3
"""Generate tests/golden/qwen3_state_dict.json: the state-dict entry names, shapes and dtypes of the installed transformers'
Qwen3ForCausalLM (cast to fp16, as a checkpoint is loaded) for one tiny config, with the config fields QuantLlamaForCausalLM.from_config
reads.  head_dim (128) differs from hidden_size / num_attention_heads (64), and the embeddings are tied.

Unlike the Llama / Qwen2 fixture (gen_causal_lm_state_dict.py: derived by reading, the reference's classes do not import), this one is
made by instantiating the class: the names of a Qwen3 checkpoint are transformers', the reference has no Qwen3 model.

usage: python tests/golden/gen_qwen3_state_dict.py      (writes tests/golden/qwen3_state_dict.json)
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

CONFIG = dict(vocab_size=1000, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=512,
              num_hidden_layers=2, rms_norm_eps=1e-6, tie_word_embeddings=True)
# what from_config reads (duck-typed), as the installed transformers' Qwen3Config spells it
FIELDS = ("model_type", "vocab_size", "hidden_size", "num_attention_heads", "num_key_value_heads", "head_dim", "intermediate_size",
          "num_hidden_layers", "rms_norm_eps", "attention_bias", "tie_word_embeddings", "hidden_act", "rope_parameters", "rope_theta",
          "rope_scaling", "use_sliding_window", "sliding_window", "layer_types")


def build():
    import torch
    from transformers import Qwen3Config, Qwen3ForCausalLM

    cfg = Qwen3Config(**CONFIG)
    with torch.device("meta"):
        model = Qwen3ForCausalLM(cfg).half()
    as_dict = cfg.to_dict()
    config = {k: as_dict[k] for k in FIELDS if k in as_dict}
    entries = {k: dict(shape=list(v.shape), dtype=str(v.dtype).replace("torch.", "")) for k, v in model.state_dict().items()}
    return dict(config=config, entries=entries)


if __name__ == "__main__":
    with open(os.path.join(HERE, "qwen3_state_dict.json"), "w") as f:
        json.dump(build(), f, indent=1, sort_keys=True)
        f.write("\n")
