"""Llama decoder-block modules around QuantLinear: the RMSNorm and the MLP of the reference's dense decoder
(QQQ/gptq/models/llama.py: LlamaRMSNorm, QuantizedLlamaMLP), with the activation in front of every GEMM produced already quantised.

    QuantRMSNorm      LlamaRMSNorm (+ the residual add in front of it) -> (xq, s1) for the q/k/v or gate/up projections, one launch
    QuantLlamaMLP     down(silu(gate(x)) * up(x)): the product is quantised in the same launch that computes it (silu_mul_quant)

Parameter and buffer names are the reference's, so `input_layernorm.*`, `post_attention_layernorm.*` and `mlp.*` state-dicts load unchanged.
Attention, RoPE, the KV cache and the whole decoder layer are in qqq_amd/attention.py (QuantLlamaAttention, QuantLlamaDecoderLayer).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .qlinear import QuantLinear, fuse_quant_linears


class QuantRMSNorm(nn.Module):
    """LlamaRMSNorm (fp16) whose output is the per-token int8 quantisation (xq, s1) the next QuantLinear.forward_int8 takes.

    forward(x) -> (xq, s1) of y = weight * fp16(float(x) * rsqrt(mean(float(x)^2) + eps)).
    forward(x, residual) -> the same of the norm of h = fp16(residual + x); `residual` is updated to h in place."""

    def __init__(self, hidden_size: int, eps: float = 1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size, dtype=torch.float16), requires_grad=False)
        self.variance_epsilon = eps

    def forward(self, x: torch.Tensor, residual: torch.Tensor = None):
        w = self.weight if self.weight.dtype == torch.float16 else self.weight.half()
        return ops.rmsnorm_quant(x, w, self.variance_epsilon, residual=residual)

    def extra_repr(self) -> str:
        return f"{self.weight.shape[0]}, eps={self.variance_epsilon}"


def _no_lora(name):
    return None


def forward_int8_lora(mod, xq: torch.Tensor, s1: torch.Tensor, lora):
    """mod.forward_int8(xq, s1), with `lora` behind them only when there is one: a call without adapters is the call it always was"""
    return mod.forward_int8(xq, s1) if lora is None else mod.forward_int8(xq, s1, lora)


def lora_add_slices(xq: torch.Tensor, s1: torch.Tensor, lora, named) -> None:
    """ops.lora_add on the column slices `named` = ((projection, its view of a fused output), ...) for which `lora` holds adapters: what a
    fused holder runs when only part of its group is targeted"""
    for name, y in named:
        g = lora(name)
        if g is not None and y.shape[0]:
            if y.dim() != 2 or xq.dim() != 2:
                raise RuntimeError("lora: adapters take packed token rows, xq [tokens, infeatures]")
            ops.lora_add(y, xq, s1.reshape(-1), *g)


def _drop_fused_on_load(module, *args, **kwargs):
    module._gate_up = None  # a state-dict is being loaded: the fused gate|up copy would be stale


class QuantLlamaMLP(nn.Module):
    """QuantizedLlamaMLP (SiLU): down_proj(silu(gate_proj(x)) * up_proj(x)) with W4A8 QuantLinears.

    forward(x) quantises the fp16 input once for both projections; forward_int8(xq, s1) takes it already quantised (QuantRMSNorm).
    The silu * up product goes straight into down_proj's int8 input (silu_mul_quant): it is never written as fp16."""

    def __init__(self, hidden_size: int, intermediate_size: int, group_size: int, bias: bool = False):
        super().__init__()
        self.hidden_size = hidden_size
        self.intermediate_size = intermediate_size
        self.gate_proj = QuantLinear(4, group_size, hidden_size, intermediate_size, bias=bias)
        self.up_proj = QuantLinear(4, group_size, hidden_size, intermediate_size, bias=bias)
        self.down_proj = QuantLinear(4, group_size, intermediate_size, hidden_size, bias=bias)
        self._gate_up = None  # fuse_gate_up(): the fused gate|up layer, kept outside the module tree (not in the state-dict)
        # a plain function, given the module by torch through a weak reference: a bound method would make module -> hook -> module a
        # reference cycle, and the module's device memory would then wait for Python's cyclic garbage collector
        self._register_load_state_dict_pre_hook(_drop_fused_on_load, with_module=True)

    @torch.no_grad()
    def fuse_gate_up(self):
        """Opt-in: ONE GEMM for gate and up (fuse_quant_linears: N = 2 * intermediate_size), whose output halves feed silu_mul_quant in
        place.  Memory: the fused layer is a second copy of gate_proj's and up_proj's weights, scales and bias (the same byte count
        again, about hidden * intermediate bytes); gate_proj and up_proj are kept as they are.  state_dict(): unchanged -- the fused
        copy is not part of it, keys stay the reference's.  Loading a state-dict drops the fused copy (it would be stale) and the
        module falls back to the two separate GEMMs until fuse_gate_up() is called again; unfuse_gate_up() releases it.  The fused
        layer follows later .to() / .cuda() moves of the module.  Returns self."""
        fused = fuse_quant_linears([self.gate_proj, self.up_proj])
        if self.gate_proj.W8 is not None and self.up_proj.W8 is not None:
            fused.expand_for_prefill(per_channel=True)
        object.__setattr__(self, "_gate_up", fused)  # a plain attribute: nn.Module would register it as a submodule
        return self

    def unfuse_gate_up(self):
        """Release the fused gate|up layer of fuse_gate_up()."""
        self._gate_up = None
        return self

    @property
    def gate_up_fused(self) -> bool:
        return self._gate_up is not None

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse=recurse)
        if self._gate_up is not None:
            self._gate_up._apply(fn, recurse=recurse)
        return self

    def forward_int8(self, xq: torch.Tensor, s1: torch.Tensor, lora=None) -> torch.Tensor:
        """`lora`: None, or the layer's LayerLora (qqq_amd/lora.py): lora(name) -> what QuantLinear.forward_int8(lora=) takes, or None"""
        pick = lora if lora is not None else _no_lora
        if self._gate_up is not None:
            gu = forward_int8_lora(self._gate_up, xq, s1, pick("gate_up"))
            i = self.intermediate_size
            gate, up = gu[..., :i], gu[..., i:]
            if lora is not None and pick("gate_up") is None:  # part of the group is targeted: its columns of the fused output
                lora_add_slices(xq, s1, lora, (("gate_proj", gate), ("up_proj", up)))
            hq, hs = ops.silu_mul_quant(gate, up)
        else:
            hq, hs = ops.silu_mul_quant(forward_int8_lora(self.gate_proj, xq, s1, pick("gate_proj")),
                                        forward_int8_lora(self.up_proj, xq, s1, pick("up_proj")))
        return forward_int8_lora(self.down_proj, hq, hs, pick("down_proj"))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward_int8(*ops.dynamic_quant(x.half()))


__all__ = ["QuantRMSNorm", "QuantLlamaMLP"]
