"""Mixture-of-experts MLP of a Qwen3-MoE or Mixtral decoder layer on the W4A8 kernels: the routing, both expert GEMMs and the combine
run on the device in a fixed number of launches, so the block sits inside a captured decode step whatever the routing.

    QuantMoeExperts       the experts' packed weights stacked: gate_up_proj (gate | up along N) and down_proj, each {B, s_channel, s_group}
    QuantSparseMoeBlock   an fp16 router `gate` and `experts`; forward_int8(xq, s1, y) is
                          F.linear(y, gate.weight) -> moe_route -> moe_gemm(a_div = top_k) -> silu_mul_quant -> moe_gemm(a_div = 1) -> moe_combine

State-dict keys under a layer's `mlp.`: gate.weight, experts.gate_up_proj.{B, s_channel, s_group}, experts.down_proj.{B, s_channel, s_group}.
The weights come from qqq_amd.quant.quantize_model (per-expert Hessians over routed calibration rows) or from QuantLinears packed
elsewhere, through load_expert.  Shared experts, LoRA on experts and expert parallelism are not here.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .qlinear import QuantLinear


class _StackedLinears(nn.Module):
    """E packed QuantLinears [K -> N] as three stacked buffers, every slice in QuantLinear's own layout and stored scale order"""

    def __init__(self, num_experts: int, infeatures: int, outfeatures: int, group_size: int):
        super().__init__()
        if infeatures % 128 or outfeatures % 64:
            raise ValueError(f"expert matrices need infeatures % 128 == 0 and outfeatures % 64 == 0, not {infeatures} -> {outfeatures}")
        if group_size not in (-1, 128):
            raise ValueError("Only group_size -1 and 128 are supported.")
        if group_size == infeatures:  # QuantLinear's rule: one group over all of K is the per-channel format, without s_group
            group_size = -1
        self.infeatures, self.outfeatures, self.group_size = infeatures, outfeatures, group_size
        self.register_buffer("B", torch.empty((num_experts, infeatures // 16, outfeatures * 2), dtype=torch.int32))
        self.register_buffer("s_channel", torch.empty((num_experts, 1, outfeatures), dtype=torch.float32))
        groups = infeatures // 128 if group_size == 128 else 0
        self.register_buffer("s_group", torch.empty((num_experts, groups, outfeatures) if groups else (0,), dtype=torch.half))

    def _apply(self, fn, recurse=True):
        # the scales keep their dtypes and values across .half() / .to(dtype), as QuantLinear's do: they only follow device moves
        keep = {"s_group": self.s_group, "s_channel": self.s_channel}
        super()._apply(fn, recurse=recurse)
        for name, old in keep.items():
            cur = getattr(self, name)
            if cur.dtype != old.dtype:
                setattr(self, name, old.to(device=cur.device))
        return self

    @torch.no_grad()
    def load(self, e: int, cols: slice, layer: QuantLinear) -> None:
        gs = -1 if layer.group_size == layer.infeatures else layer.group_size
        n = cols.stop - cols.start
        if layer.infeatures != self.infeatures or layer.outfeatures != n or gs != self.group_size or layer.bias is not None:
            raise ValueError(f"load_expert: expected a bias-free QuantLinear {self.infeatures} -> {n} with group_size {self.group_size}")
        self.B[e, :, 2 * cols.start:2 * cols.stop] = layer.B.to(self.B.device)
        self.s_channel[e, :, cols] = layer.s_channel.to(self.s_channel.device)
        if self.s_group.numel():
            self.s_group[e, :, cols] = layer.s_group.to(self.s_group.device)


class QuantMoeExperts(nn.Module):
    """The experts of one layer: gate_up_proj [E, hidden -> 2 * intermediate] holds gate | up along N -- the concatenation
    fuse_quant_linears([gate, up]) makes -- and down_proj [E, intermediate -> hidden]."""

    def __init__(self, num_experts: int, hidden: int, intermediate: int, group_size: int):
        super().__init__()
        self.num_experts, self.hidden_size, self.intermediate_size = num_experts, hidden, intermediate
        self.gate_up_proj = _StackedLinears(num_experts, hidden, 2 * intermediate, group_size)
        self.down_proj = _StackedLinears(num_experts, intermediate, hidden, group_size)

    def load_expert(self, e: int, gate: QuantLinear, up: QuantLinear, down: QuantLinear) -> None:
        """copy three packed QuantLinears in as expert e"""
        i = self.intermediate_size
        self.gate_up_proj.load(e, slice(0, i), gate)
        self.gate_up_proj.load(e, slice(i, 2 * i), up)
        self.down_proj.load(e, slice(0, self.hidden_size), down)


class QuantSparseMoeBlock(nn.Module):
    """Qwen3MoeSparseMoeBlock / MixtralSparseMoeBlock: softmax router over `num_experts`, `top_k` SiLU experts per token, their outputs
    weighted by the routing probabilities (renormalised over the chosen ones with `norm_topk_prob`) and summed.

    forward_int8(xq, s1, y): (xq, s1) the quantised normed hidden rows the experts consume, y the same rows in fp16 for the router
    (QuantRMSNorm(..., return_y=True) gives all three).  Seven launches, whatever the routing; nothing is read on the host."""

    def __init__(self, hidden: int, moe_intermediate: int, num_experts: int, top_k: int, norm_topk_prob: bool, group_size: int):
        super().__init__()
        if not 2 <= num_experts <= 256 or not 1 <= top_k <= min(num_experts, 16):
            raise ValueError(f"num_experts {num_experts} and top_k {top_k}: need 2 <= num_experts <= 256 and 1 <= top_k <= min(num_experts, 16)")
        self.hidden_size, self.intermediate_size = hidden, moe_intermediate
        self.num_experts, self.top_k, self.norm_topk_prob, self.group_size = num_experts, top_k, bool(norm_topk_prob), group_size
        self.gate = nn.Linear(hidden, num_experts, bias=False, dtype=torch.float16)
        self.gate.weight.requires_grad_(False)
        self.experts = QuantMoeExperts(num_experts, hidden, moe_intermediate, group_size)

    def forward_int8(self, xq: torch.Tensor, s1: torch.Tensor, y: torch.Tensor, lora=None) -> torch.Tensor:
        if lora is not None:
            raise NotImplementedError("QuantSparseMoeBlock: LoRA on experts is not supported")
        if xq.dtype != torch.int8 or xq.shape[-1] != self.hidden_size or y.shape != xq.shape:
            raise RuntimeError(f"forward_int8: xq must be int8 [..., {self.hidden_size}] and y the fp16 rows of the same shape")
        out_shape = xq.shape
        xq, y, s1 = xq.reshape(-1, self.hidden_size).contiguous(), y.reshape(-1, self.hidden_size), s1.reshape(-1).contiguous()
        if xq.shape[0] == 0:
            return y.new_empty(out_shape)
        k, ex = self.top_k, self.experts
        gu_gs, down_gs = ex.gate_up_proj.group_size, ex.down_proj.group_size
        ids, w, offsets, order = ops.moe_route(F.linear(y, self.gate.weight), k, self.norm_topk_prob)
        gu = ops.moe_gemm(xq, s1, ex.gate_up_proj.B, ex.gate_up_proj.s_channel, ex.gate_up_proj.s_group, ids, offsets, order, k, k, gu_gs)
        i = self.intermediate_size
        hq, hs = ops.silu_mul_quant(gu[:, :i], gu[:, i:])
        d = ops.moe_gemm(hq, hs.reshape(-1), ex.down_proj.B, ex.down_proj.s_channel, ex.down_proj.s_group, ids, offsets, order, k, 1, down_gs)
        return ops.moe_combine(d, w, k).reshape(out_shape)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = x.half()
        return self.forward_int8(*ops.dynamic_quant(y), y)


__all__ = ["QuantMoeExperts", "QuantSparseMoeBlock"]
