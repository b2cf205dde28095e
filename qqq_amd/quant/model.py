"""GPTQ over a whole Llama / Qwen2 checkpoint: the reference's layer-wise flow (QQQ/gptq/models/llama.py, gptq_llama_func) over a small fp16
float decoder layer written here -- transformers is not imported.  The inputs of layer 0 are the embedded calibration tokens; every layer
accumulates the Hessians of its linears' inputs with its FLOAT weights (all seven in one pass, as the reference), is quantised, and runs
once more with the quantised weights to feed the next layer."""
from __future__ import annotations

import copy
from typing import Optional

import torch
import torch.nn.functional as F

from ..attention import _config_rope, rope_inv_freq, rope_tables
from ..model import QuantLlamaForCausalLM
from .gptq import Hessian, gptq_quantize, gptq_quantize_ordered
from .rotation import rotate_model

ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
MLP = ("gate_proj", "up_proj", "down_proj")
# the Hessian every linear is quantised under: one per distinct input
HESSIAN_OF = {"q_proj": "qkv", "k_proj": "qkv", "v_proj": "qkv", "o_proj": "o", "gate_proj": "gate_up", "up_proj": "gate_up", "down_proj": "down"}


def _rms_norm(x, weight, eps):
    h = x.float()
    h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)
    return weight * h.to(x.dtype)


def _rotate_half(x):
    half = x.shape[-1] // 2
    return torch.cat((-x[..., half:], x[..., :half]), dim=-1)


class FloatDecoderLayer:
    """transformers' Llama / Qwen2 decoder layer in fp16 from plain tensors: RMSNorm, RoPE (rope_tables), causal SDPA, SiLU MLP.
    `weights`: {"self_attn.q_proj.weight": ..., "mlp.down_proj.weight": ..., "input_layernorm.weight": ..., optional "...bias"} on one
    device.  forward(x [b, s, hidden], taps=None): `taps` maps "qkv" / "o" / "gate_up" / "down" to a callable that sees that input."""

    def __init__(self, config, weights: dict):
        self.w = weights
        self.heads = config.num_attention_heads
        self.kv_heads = getattr(config, "num_key_value_heads", None) or self.heads
        self.head_dim = getattr(config, "head_dim", None) or config.hidden_size // self.heads
        self.eps = config.rms_norm_eps
        theta, rope = _config_rope(config)
        self.inv_freq, self.attention_scaling = rope_inv_freq(self.head_dim, theta, rope)
        self._tables = None

    def _linear(self, name, x):
        return F.linear(x, self.w[name + ".weight"], self.w.get(name + ".bias"))

    def _rope(self, length, device):
        if self._tables is None or self._tables[0].shape[0] < length or self._tables[0].device != device:
            self._tables = rope_tables(self.inv_freq, self.attention_scaling, length, device)
        return self._tables[0][:length], self._tables[1][:length]

    @torch.no_grad()
    def forward(self, x: torch.Tensor, taps: Optional[dict] = None) -> torch.Tensor:
        taps = taps or {}
        b, s, _ = x.shape
        h = _rms_norm(x, self.w["input_layernorm.weight"], self.eps)
        if "qkv" in taps:
            taps["qkv"](h)
        q = self._linear("self_attn.q_proj", h).view(b, s, self.heads, self.head_dim).transpose(1, 2)
        k = self._linear("self_attn.k_proj", h).view(b, s, self.kv_heads, self.head_dim).transpose(1, 2)
        v = self._linear("self_attn.v_proj", h).view(b, s, self.kv_heads, self.head_dim).transpose(1, 2)
        if "self_attn.q_norm.weight" in self.w:  # Qwen3: RMSNorm over head_dim between the q / k projections and RoPE
            q = _rms_norm(q, self.w["self_attn.q_norm.weight"], self.eps)
            k = _rms_norm(k, self.w["self_attn.k_norm.weight"], self.eps)
        cos, sin = self._rope(s, x.device)
        q = q * cos + _rotate_half(q) * sin
        k = k * cos + _rotate_half(k) * sin
        rep = self.heads // self.kv_heads
        if rep > 1:
            k, v = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
        a = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(b, s, self.heads * self.head_dim)
        if "o" in taps:
            taps["o"](a)
        x = x + self._linear("self_attn.o_proj", a)
        h = _rms_norm(x, self.w["post_attention_layernorm.weight"], self.eps)
        if "gate_up" in taps:
            taps["gate_up"](h)
        m = F.silu(self._linear("mlp.gate_proj", h)) * self._linear("mlp.up_proj", h)
        if "down" in taps:
            taps["down"](m)
        return x + self._linear("mlp.down_proj", m)


def _run(layer, inps, seq_batch, taps=None):
    return torch.cat([layer.forward(inps[j:j + seq_batch], taps) for j in range(0, inps.shape[0], seq_batch)], dim=0)


@torch.no_grad()
def quantize_model(state_dict: dict, config, calib_ids: torch.Tensor, group_size: int, mse: bool = False, percdamp: float = 0.01,
                   seq_batch: int = 1, device=None, results: Optional[dict] = None, rotation=None, act_order: bool = False,
                   static_groups: bool = False, smooth=None) -> QuantLlamaForCausalLM:
    """A packed QuantLlamaForCausalLM from an fp16 Hugging Face state dict, a (duck-typed) Llama or Qwen2 config and calibration token
    ids [samples, seqlen].  `seq_batch` sequences run through a layer at a time (1, the reference's, counts every sequence as one sample
    of the Hessian).  `results`: a dict that receives the GPTQResult of every linear under its state-dict prefix.
    `rotation`: None, or what rotation.rotate_model is to do to the state dict first (the reference's --rotation; pair it with mse=True):
    "hadamard", "hadamard_k" (hidden sizes K * 2^p), "random", an int8 [hidden] sign vector, an f64 [hidden, hidden] Q, or the pair
    ("hadamard_k", signs).  The model is then built UNTIED (its lm_head carries the final norm), its norms are ones, and
    results["rotation"] receives the signs or Q that were used.
    `act_order`, `static_groups`: the reference's --gptq_act_order / --gptq_static_groups (both on by default THERE, off here): with
    either, every linear goes through gptq_quantize_ordered; groups with act_order need static_groups too.  The checkpoint's layout does
    not change.
    `smooth`: None, a method name ("os+", "awq", "sq": smooth.smooth_model searches the scales on the first 8 calibration sequences), or
    a ready scale_list (smooth.apply_smooth alone): the reference's --smooth True (pair it with mse=False).  It is applied AFTER
    `rotation`, on the rotated state dict, and before GPTQ; results["smooth"] receives the list.  After rotation + smooth the norms are
    no longer ones: they hold 1 / s.  With smooth=None nothing of it runs."""
    dev = torch.device(device if device is not None else "cuda:0")
    if rotation is not None:
        if isinstance(rotation, str):
            kw = dict(mode=rotation)
        elif isinstance(rotation, torch.Tensor):
            kw = dict(signs=rotation) if rotation.dtype == torch.int8 else dict(Q=rotation)
        elif isinstance(rotation, tuple) and len(rotation) == 2 and rotation[0] == "hadamard_k" and isinstance(rotation[1], torch.Tensor):
            kw = dict(mode="hadamard_k", signs=rotation[1])
        else:
            raise RuntimeError("quantize_model: rotation must be None, 'hadamard', 'hadamard_k', 'random', a tensor (signs or Q) or "
                               f"('hadamard_k', signs), got {type(rotation).__name__}")
        state_dict, used = rotate_model(state_dict, config, device=dev, **kw)
        config = copy.copy(config)
        config.tie_word_embeddings = False
        if results is not None:
            results["rotation"] = used
    if smooth is not None:
        from . import smooth as _smooth

        if isinstance(smooth, str):
            if smooth not in _smooth.METHODS:
                raise RuntimeError(f"quantize_model: smooth must be None, one of {_smooth.METHODS} or a scale_list, got {smooth!r}")
            state_dict, scale_list = _smooth.smooth_model(state_dict, config, calib_ids, group_size, method=smooth, device=dev)
        elif isinstance(smooth, (list, tuple)):
            scale_list = list(smooth)
            state_dict = _smooth.apply_smooth(state_dict, config, scale_list)
        else:
            raise RuntimeError(f"quantize_model: smooth must be None, one of {_smooth.METHODS} or a scale_list, got {type(smooth).__name__}")
        if results is not None:
            results["smooth"] = scale_list
    lm = QuantLlamaForCausalLM.from_config(config, group_size).to(dev)
    embed = state_dict["model.embed_tokens.weight"].to(dev).half()
    ids = torch.as_tensor(calib_ids, dtype=torch.int64, device=dev)
    if ids.dim() != 2:
        raise RuntimeError("quantize_model: calib_ids must be [samples, seqlen] token ids")
    inps = F.embedding(ids, embed)
    for i, qlayer in enumerate(lm.model.layers):
        prefix = f"model.layers.{i}."
        w = {k[len(prefix):]: v.to(dev).half() for k, v in state_dict.items() if k.startswith(prefix)}
        layer = FloatDecoderLayer(config, w)
        hidden, inter = w["mlp.gate_proj.weight"].shape[1], w["mlp.down_proj.weight"].shape[1]
        hs = {"qkv": Hessian(hidden, dev), "o": Hessian(w["self_attn.o_proj.weight"].shape[1], dev), "gate_up": Hessian(hidden, dev),
              "down": Hessian(inter, dev)}
        _run(layer, inps, seq_batch, {k: h.add_batch for k, h in hs.items()})
        for mod_name, names in (("self_attn", ATTN), ("mlp", MLP)):
            for name in names:
                key = f"{mod_name}.{name}"
                W = w[key + ".weight"]
                if act_order or static_groups:
                    res = gptq_quantize_ordered(W, hs[HESSIAN_OF[name]].H, group_size, mse=mse, percdamp=percdamp, act_order=act_order,
                                                static_groups=static_groups)
                else:
                    res = gptq_quantize(W, hs[HESSIAN_OF[name]].H, group_size, mse=mse, percdamp=percdamp)
                res.pack_into(getattr(getattr(qlayer, mod_name), name), w.get(key + ".bias"))
                w[key + ".weight"] = res.weight
                if results is not None:
                    results[prefix + key] = res
        qlayer.input_layernorm.weight.data.copy_(w["input_layernorm.weight"])
        qlayer.post_attention_layernorm.weight.data.copy_(w["post_attention_layernorm.weight"])
        if qlayer.self_attn.qk_norm:  # Qwen3: the per-head norms go into the packed model as they are
            qlayer.self_attn.q_norm.weight.data.copy_(w["self_attn.q_norm.weight"])
            qlayer.self_attn.k_norm.weight.data.copy_(w["self_attn.k_norm.weight"])
        inps = _run(layer, inps, seq_batch)
        del hs
    lm.model.embed_tokens.weight.data.copy_(embed)
    lm.model.norm.weight.data.copy_(state_dict["model.norm.weight"].to(dev))
    if "lm_head.weight" in state_dict:
        lm.lm_head.weight.data.copy_(state_dict["lm_head.weight"].to(dev))
    elif lm.lm_head.weight is not lm.model.embed_tokens.weight:
        lm.lm_head.weight.data.copy_(embed)
    return lm.eval()
