"""GPTQ over a whole Llama / Qwen2 checkpoint: the reference's layer-wise flow (QQQ/gptq/models/llama.py, gptq_llama_func) over a small fp16
float decoder layer written here -- transformers is not imported.  The inputs of layer 0 are the embedded calibration tokens; every layer
accumulates the Hessians of its linears' inputs with its FLOAT weights (all seven in one pass, as the reference), is quantised, and runs
once more with the quantised weights to feed the next layer.  A sparse (mixture-of-experts) layer of Qwen3-MoE or Mixtral keeps one
Hessian per expert and input, over the rows the router sends there (ExpertHessians), and quantises every expert under its own."""
from __future__ import annotations

import copy
from typing import Optional

import torch
import torch.nn.functional as F

from ..attention import _config_rope, rope_inv_freq, rope_tables
from ..model import QuantLlamaForCausalLM
from .. import ops as _serve_ops
from ..qlinear import QuantLinear
from .gptq import ExpertHessians, Hessian, gptq_quantize, gptq_quantize_experts, gptq_quantize_ordered
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
    device.  forward(x [b, s, hidden], taps=None): `taps` maps "qkv" / "o" / "gate_up" / "down" to a callable that sees that input.
    With "mlp.gate.weight" among the weights the MLP is the sparse block of Qwen3-MoE / Mixtral over "mlp.experts.E.{gate,up,down}_proj":
    routed by ops.moe_route as inference routes, the experts a torch loop over gathered rows; its "gate_up" and "down" taps are called
    with (rows, offsets, order): the flat normed rows [tokens, hidden], then the SiLU-mul rows [tokens * top_k, intermediate] in pair order."""

    def __init__(self, config, weights: dict):
        self.w = weights
        self.heads = config.num_attention_heads
        self.kv_heads = getattr(config, "num_key_value_heads", None) or self.heads
        self.head_dim = getattr(config, "head_dim", None) or config.hidden_size // self.heads
        self.eps = config.rms_norm_eps
        theta, rope = _config_rope(config)
        self.inv_freq, self.attention_scaling = rope_inv_freq(self.head_dim, theta, rope)
        self._tables = None
        self.sparse = "mlp.gate.weight" in weights
        if self.sparse:
            self.num_experts = weights["mlp.gate.weight"].shape[0]
            self.top_k = config.num_experts_per_tok
            self.renorm = getattr(config, "model_type", "") == "mixtral" or bool(getattr(config, "norm_topk_prob", False))

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
        if self.sparse:
            return x + self._sparse_mlp(h, taps)
        if "gate_up" in taps:
            taps["gate_up"](h)
        m = F.silu(self._linear("mlp.gate_proj", h)) * self._linear("mlp.up_proj", h)
        if "down" in taps:
            taps["down"](m)
        return x + self._linear("mlp.down_proj", m)


    def _sparse_mlp(self, h, taps):
        k = self.top_k
        flat = h.reshape(-1, h.shape[-1])
        _, weights, offsets, order = _serve_ops.moe_route(F.linear(flat, self.w["mlp.gate.weight"]), k, self.renorm)
        if "gate_up" in taps:
            taps["gate_up"](flat, offsets, order)
        offs = offsets.tolist()  # the one host read of the routing
        pairs = [order[offs[e]:offs[e + 1]].long() for e in range(self.num_experts)]
        m = torch.empty((order.numel(), self.w["mlp.experts.0.down_proj.weight"].shape[1]), dtype=h.dtype, device=h.device)
        for e, p in enumerate(pairs):
            if p.numel():
                rows = flat[p // k]
                m[p] = F.silu(self._linear(f"mlp.experts.{e}.gate_proj", rows)) * self._linear(f"mlp.experts.{e}.up_proj", rows)
        if "down" in taps:
            taps["down"](m, offsets, order)
        d = torch.empty((order.numel(), h.shape[-1]), dtype=h.dtype, device=h.device)
        for e, p in enumerate(pairs):
            if p.numel():
                d[p] = self._linear(f"mlp.experts.{e}.down_proj", m[p])
        return _serve_ops.moe_combine(d, weights, k).reshape(h.shape)


_MIXTRAL_KEYS = ((".block_sparse_moe.gate.", ".mlp.gate."), (".w1.", ".gate_proj."), (".w3.", ".up_proj."), (".w2.", ".down_proj."),
                 (".block_sparse_moe.experts.", ".mlp.experts."))


def _qwen3_moe_keys(state_dict):
    """Mixtral's names of the sparse block mapped onto Qwen3-MoE's, which the packed model and everything below use"""
    out = {}
    for key, v in state_dict.items():
        if ".block_sparse_moe." in key:
            for old, new in _MIXTRAL_KEYS:
                key = key.replace(old, new)
        out[key] = v
    return out


def _run(layer, inps, seq_batch, taps=None):
    return torch.cat([layer.forward(inps[j:j + seq_batch], taps) for j in range(0, inps.shape[0], seq_batch)], dim=0)


@torch.no_grad()
def quantize_model(state_dict: dict, config, calib_ids: torch.Tensor, group_size: int, mse: bool = False, percdamp: float = 0.01,
                   seq_batch: int = 1, device=None, results: Optional[dict] = None, rotation=None, act_order: bool = False,
                   static_groups: bool = False, smooth=None, factor: str = "torch", hessian: str = "torch") -> QuantLlamaForCausalLM:
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
    no longer ones: they hold 1 / s.  With smooth=None nothing of it runs.
    `factor`: "torch" or "fused", handed to every linear's gptq_quantize / gptq_quantize_ordered (the factor of the inverse Hessian from
    torch's Cholesky chain, or from ops.upper_factor).
    `hessian`: "torch" or "fused", handed to the four Hessians of every layer as their `accumulate` (the reference's f32 steps, or
    ops.hessian_update on the fp16 taps; for a sparse layer's experts, ExpertHessians' per-expert loop or ops.hessian_update_grouped).
    A `qwen3_moe` or `mixtral` config: Mixtral's state-dict names (block_sparse_moe.gate, experts.E.w1 / w3 / w2) are mapped onto
    Qwen3-MoE's on entry; every expert linear is quantised under its own Hessian over the rows routed to it (an expert that saw none:
    round-to-nearest, gptq_quantize_experts) and loaded with load_expert; the router is copied.  `results` also receives, under
    "model.layers.N.mlp.experts", {"gate_up": count, "down": count, "fallback": [experts]} -- the rows every expert saw.  `rotation` and
    `smooth` with a sparse model raise NotImplementedError: neither folds into routed experts yet."""
    dev = torch.device(device if device is not None else "cuda:0")
    state_dict = _qwen3_moe_keys(state_dict)
    if (rotation is not None or smooth is not None) and any(k.endswith(".mlp.gate.weight") for k in state_dict):
        raise NotImplementedError("quantize_model: rotation and smooth are not supported for mixture-of-experts models (sparse layers)")
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
        hidden = w["self_attn.q_proj.weight"].shape[1]
        hs = {"qkv": Hessian(hidden, dev, hessian), "o": Hessian(w["self_attn.o_proj.weight"].shape[1], dev, hessian)}
        taps = {k: h.add_batch for k, h in hs.items()}
        if layer.sparse:
            E, top_k, inter = layer.num_experts, layer.top_k, w["mlp.experts.0.down_proj.weight"].shape[1]
            xh = {"gate_up": ExpertHessians(E, hidden, dev, hessian), "down": ExpertHessians(E, inter, dev, hessian)}
            taps["gate_up"] = lambda x, offsets, order: xh["gate_up"].add_batch(x, offsets, order, top_k)
            taps["down"] = lambda x, offsets, order: xh["down"].add_batch(x, offsets, order, 1)
        else:
            hs.update(gate_up=Hessian(hidden, dev, hessian), down=Hessian(w["mlp.down_proj.weight"].shape[1], dev, hessian))
            taps = {k: h.add_batch for k, h in hs.items()}
        _run(layer, inps, seq_batch, taps)
        if layer.sparse:
            fallback, packed = [], {}
            for name in MLP:
                W = torch.stack([w[f"mlp.experts.{e}.{name}.weight"] for e in range(E)])
                eh = xh[HESSIAN_OF[name]]
                gs = -1 if group_size == W.shape[2] else group_size  # (one group over all of K is QuantLinear's per-channel format)
                found = []
                for e, res in enumerate(gptq_quantize_experts(W, eh.H, eh.count, gs, mse=mse, percdamp=percdamp, act_order=act_order,
                                                              static_groups=static_groups, factor=factor, fallback=found)):
                    packed[e, name] = res.pack_into(QuantLinear(4, gs, W.shape[2], W.shape[1], False).to(dev))
                    w[f"mlp.experts.{e}.{name}.weight"] = res.weight
                    if results is not None:
                        results[f"{prefix}mlp.experts.{e}.{name}"] = res
                fallback = sorted(set(fallback) | set(found))
            for e in range(E):
                qlayer.mlp.experts.load_expert(e, *(packed[e, name] for name in MLP))
            qlayer.mlp.gate.weight.data.copy_(w["mlp.gate.weight"])
            if results is not None:
                results[prefix + "mlp.experts"] = {"gate_up": xh["gate_up"].count, "down": xh["down"].count, "fallback": fallback}
            del xh, packed
        for mod_name, names in (("self_attn", ATTN), ("mlp", () if layer.sparse else MLP)):
            for name in names:
                key = f"{mod_name}.{name}"
                W = w[key + ".weight"]
                if act_order or static_groups:
                    res = gptq_quantize_ordered(W, hs[HESSIAN_OF[name]].H, group_size, mse=mse, percdamp=percdamp, act_order=act_order,
                                                static_groups=static_groups, factor=factor)
                else:
                    res = gptq_quantize(W, hs[HESSIAN_OF[name]].H, group_size, mse=mse, percdamp=percdamp, factor=factor)
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
