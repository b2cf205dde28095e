"""GPTQ for one linear layer on the device: the reference's `GPTQ.add_batch` and `GPTQ.fasterquant` (QQQ/gptq/gptq.py) in their order, with
the two launch-bound pieces -- the scale search and the column sweep of a block -- as one HIP launch each (qqq_amd/quant/ops.py).  The
Hessian, the three Cholesky steps and the trailing GEMM between blocks stay in torch: they are a few large launches.

Only what QuantLinear.pack can hold: symmetric 4-bit, per-channel (group_size -1) or groups of 128.  No act-order, no static groups."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional

import torch

from . import ops

BLOCK = 128


class Hessian:
    """The running 2/n X^T X of a linear layer's inputs, as the reference accumulates it (f32 [columns, columns])."""

    def __init__(self, columns: int, device):
        self.columns = columns
        self.H = torch.zeros((columns, columns), dtype=torch.float32, device=device)
        self.nsamples = 0

    @torch.no_grad()
    def add_batch(self, x: torch.Tensor) -> None:
        """`x` [..., columns]: a 2-D input counts as one sample, a 3-D one as its leading dimension (what the reference counts)"""
        if x.shape[-1] != self.columns:
            raise RuntimeError(f"Hessian.add_batch: the input's last dimension is {x.shape[-1]}, {self.columns} expected")
        b = 1 if x.dim() <= 2 else x.shape[0]
        x = x.reshape(-1, self.columns)
        self.H *= self.nsamples / (self.nsamples + b)
        self.nsamples += b
        x = math.sqrt(2 / self.nsamples) * x.float()
        self.H += x.t().matmul(x)


class BlockTrace(NamedTuple):
    """one block of a traced run: the block as it entered the sweep, the sweep's outputs and the scale it used"""
    start: int
    block_in: torch.Tensor
    Q1: torch.Tensor
    Err1: torch.Tensor
    scale: torch.Tensor


class GPTQResult(NamedTuple):
    weight: torch.Tensor             # the fake-quantised weight [N, K] in the layer's dtype
    scales: torch.Tensor             # f32 [N, 1] per-channel, [N, K / 128] grouped
    s_extra: Optional[torch.Tensor]  # f32 [N, 1]: max |row| / 127 of `weight`, grouped only
    loss: float                      # sum Err1^2 / 2, a diagnostic
    trace: Optional[List[BlockTrace]] = None
    Hinv: Optional[torch.Tensor] = None  # with trace: the upper Cholesky factor the sweep read

    @property
    def grouped(self) -> bool:
        return self.s_extra is not None

    def codes(self) -> torch.Tensor:
        """the integer codes [N, K] the weight stands for (int8): -7 ... 7 per-channel, 0 ... 15 grouped -- what pack() stores"""
        w = self.weight.float()
        if self.grouped:
            s = self.scales.repeat_interleave(BLOCK, dim=1)
            return torch.clamp(torch.round(w / s) + 8, 0, 15).to(torch.int8)
        return torch.clamp(torch.round(w / self.scales), -7, 7).to(torch.int8)

    @torch.no_grad()
    def pack_into(self, qlinear, bias: Optional[torch.Tensor] = None):
        """QuantLinear.pack with this result (the layer's group size must be the result's).  Returns the layer."""
        if (qlinear.group_size != qlinear.infeatures) != self.grouped:
            raise RuntimeError("GPTQResult.pack_into: the layer's group size is not the one this weight was quantised for")
        qlinear.pack(_Linear(self.weight, bias), self.scales, self.s_extra)
        return qlinear


class _Linear:
    # what QuantLinear.pack reads of an nn.Linear
    def __init__(self, weight, bias):
        self.weight = _Data(weight)
        self.bias = None if bias is None else _Data(bias)


class _Data:
    def __init__(self, t):
        self.data, self.dtype = t, t.dtype


def _quantise(w, scale, grouped):
    if grouped:
        return scale * (torch.clamp(torch.round(w / scale) + 8, 0, 15) - 8)
    return scale * torch.clamp(torch.round(w / scale), -7, 7)


def _block_composed(W1, Hinv1, scale, grouped):
    """the sweep as the reference composes it from torch calls, a handful of launches per column: the baseline of `fused`"""
    W1 = W1.clone()
    Q1, Err1 = torch.zeros_like(W1), torch.zeros_like(W1)
    for i in range(W1.shape[1]):
        w, d = W1[:, i], Hinv1[i, i]
        q = _quantise(w.unsqueeze(1), scale, grouped).flatten()
        Q1[:, i] = q
        err1 = (w - q) / d
        W1[:, i:] -= err1.unsqueeze(1) * Hinv1[i, i:].unsqueeze(0)
        Err1[:, i] = err1
    return Q1, Err1


@torch.no_grad()
def gptq_quantize(W: torch.Tensor, H: torch.Tensor, group_size: int = -1, mse: bool = False, percdamp: float = 0.01, fused: bool = True,
                  trace: bool = False, bits: int = 4, sym: bool = True, act_order: bool = False, static_groups: bool = False,
                  timers=None) -> GPTQResult:
    """GPTQ of one weight `W` [N, K] (on the GPU, any float dtype) under the Hessian `H` f32 [K, K] (Hessian.H; not modified).
    group_size -1: per-channel scales found from the whole row before dead columns are zeroed; 128: a group's scale found from the
    block as it stands when the sweep reaches it.  fused=False runs the sweep as torch calls (same bits, the benchmark's baseline).
    trace=True keeps every block's input, outputs and scale, and the factor.  `timers`: None, or an object whose section(name) returns a
    context manager (tools/bench_gptq.py splits the time with it)."""
    if bits != 4 or not sym or act_order or static_groups:
        raise NotImplementedError("gptq_quantize: only symmetric 4-bit without act_order / static_groups (what QuantLinear.pack holds)")
    if group_size not in (-1, BLOCK):
        raise NotImplementedError("gptq_quantize: only group_size -1 and 128 are supported")
    if W.dim() != 2 or not W.is_cuda:
        raise RuntimeError("gptq_quantize: W must be a matrix on the GPU (there is no CPU path)")
    N, K = W.shape
    grouped = group_size == BLOCK
    if H.shape != (K, K) or H.dtype != torch.float32 or H.device != W.device:
        raise RuntimeError(f"gptq_quantize: H must be float32 [{K}, {K}] on W's device")
    if K % 64 or (grouped and K % BLOCK):
        raise RuntimeError(f"gptq_quantize: K={K} must be a multiple of 64 (of 128 when grouped): QuantLinear's admission rule")
    section = timers.section if timers is not None else _no_section

    Wf = W.float().clone()
    with section("scales"):
        scale = None if grouped else ops.weight_scales(Wf, False, mse)
    H = H.clone()
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    Wf[:, dead] = 0
    with section("cholesky"):
        damp = percdamp * torch.mean(torch.diag(H))
        diag = torch.arange(K, device=W.device)
        H[diag, diag] += damp
        H = torch.linalg.cholesky(H)
        H = torch.cholesky_inverse(H)
        Hinv = torch.linalg.cholesky(H, upper=True).contiguous()  # (the upper factor may come back as a transposed view)
    Q = torch.empty_like(Wf)
    Err1_buf = torch.empty((N, BLOCK), dtype=torch.float32, device=W.device)
    loss = torch.zeros((), dtype=torch.float32, device=W.device)
    group_scales, blocks = [], []
    for i1 in range(0, K, BLOCK):
        i2 = min(i1 + BLOCK, K)
        W1, Hinv1 = Wf[:, i1:i2], Hinv[i1:i2, i1:i2]
        if grouped:
            with section("scales"):
                scale = ops.weight_scales(W1, True, mse)
            group_scales.append(scale)
        with section("sweep"):
            if fused:
                Q1, Err1 = ops.gptq_block(W1, Hinv1, scale, grouped, out=(Q[:, i1:i2], Err1_buf[:, :i2 - i1]))
            else:
                Q1, Err1 = _block_composed(W1, Hinv1, scale, grouped)
                Q[:, i1:i2] = Q1
        loss += (Err1 * Err1).sum() / 2
        if trace:
            blocks.append(BlockTrace(i1, W1.clone(), Q1.clone(), Err1.clone(), scale.clone()))
        if i2 < K:
            with section("gemm"):
                Wf[:, i2:] -= Err1.matmul(Hinv[i1:i2, i2:])
    weight = Q.to(W.dtype)
    s_extra = None
    if grouped:
        xmax = weight.float().abs().amax(dim=1, keepdim=True)
        s_extra = torch.where(xmax == 0, torch.ones_like(xmax), xmax) / 127
    return GPTQResult(weight, torch.cat(group_scales, dim=1) if grouped else scale, s_extra, float(loss), blocks if trace else None,
                      Hinv if trace else None)


@torch.no_grad()
def round_to_nearest(W: torch.Tensor, scales: torch.Tensor, grouped: bool) -> GPTQResult:
    """`W` [N, K] rounded to the nearest code under given scales ([N, 1] per-channel, [N, K / 128] grouped), with no error feedback: the
    yardstick GPTQ is measured against"""
    s = scales.repeat_interleave(BLOCK, dim=1) if grouped else scales
    weight = _quantise(W.float(), s, grouped).to(W.dtype)
    s_extra = None
    if grouped:
        xmax = weight.float().abs().amax(dim=1, keepdim=True)
        s_extra = torch.where(xmax == 0, torch.ones_like(xmax), xmax) / 127
    return GPTQResult(weight, scales, s_extra, 0.0)


class _NoSection:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _no_section(name):
    return _NoSection()
