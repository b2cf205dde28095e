"""GPTQ for one linear layer on the device: the reference's `GPTQ.add_batch` and `GPTQ.fasterquant` (QQQ/gptq/gptq.py) in their order, with
the two launch-bound pieces -- the scale search and the column sweep of a block -- as one HIP launch each (qqq_amd/quant/ops.py).  The
Hessian, the three Cholesky steps and the trailing GEMM between blocks stay in torch: they are a few large launches.

Only what QuantLinear.pack can hold: symmetric 4-bit, per-channel (group_size -1) or groups of 128.  gptq_quantize is the plain flow;
gptq_quantize_ordered adds the reference's act-order (columns swept by falling diag(H)) and static groups (every group's scale found
before the sweep), which together still give contiguous groups: an ordinary QQQ checkpoint."""
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
    """one block of a traced run: the block as it entered the sweep, the sweep's outputs and the scale it used ([N, 1], or from
    gptq_quantize_ordered's grouped sweep the [N, count] table of per-column scales; `start` and `block_in` are then in the swept order)"""
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
    perm: Optional[torch.Tensor] = None  # gptq_quantize_ordered with act_order: the order the columns were swept in (int64 [K])

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


def _upper_factor(H, percdamp):
    """the reference's damping and three Cholesky steps on `H` (modified in place) -> the upper factor of its inverse"""
    damp = percdamp * torch.mean(torch.diag(H))
    diag = torch.arange(H.shape[0], device=H.device)
    H[diag, diag] += damp
    H = torch.linalg.cholesky(H)
    H = torch.cholesky_inverse(H)
    return torch.linalg.cholesky(H, upper=True).contiguous()  # (the upper factor may come back as a transposed view)


def _s_extra(weight):
    """f32 [N, 1]: max |row| / 127 of the fake-quantised weight (1 / 127 for an all-zero row), the grouped modes' second scale"""
    xmax = weight.float().abs().amax(dim=1, keepdim=True)
    return torch.where(xmax == 0, torch.ones_like(xmax), xmax) / 127


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
        Hinv = _upper_factor(H, percdamp)
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
    s_extra = _s_extra(weight) if grouped else None
    return GPTQResult(weight, torch.cat(group_scales, dim=1) if grouped else scale, s_extra, float(loss), blocks if trace else None,
                      Hinv if trace else None)


def _block_cols_composed(W1, Hinv1, scale_cols):
    """_block_composed in grouped arithmetic with a scale per (row, column), `scale_cols` [N, count]"""
    W1 = W1.clone()
    Q1, Err1 = torch.zeros_like(W1), torch.zeros_like(W1)
    for i in range(W1.shape[1]):
        w, d = W1[:, i], Hinv1[i, i]
        q = _quantise(w.unsqueeze(1), scale_cols[:, i:i + 1], True).flatten()
        Q1[:, i] = q
        err1 = (w - q) / d
        W1[:, i:] -= err1.unsqueeze(1) * Hinv1[i, i:].unsqueeze(0)
        Err1[:, i] = err1
    return Q1, Err1


@torch.no_grad()
def gptq_quantize_ordered(W: torch.Tensor, H: torch.Tensor, group_size: int = -1, mse: bool = False, percdamp: float = 0.01,
                          act_order: bool = True, static_groups: bool = True, perm: Optional[torch.Tensor] = None, fused: bool = True,
                          trace: bool = False, timers=None) -> GPTQResult:
    """gptq_quantize with the reference's act_order and static_groups (the defaults of its examples/quant_model.py), in the order of
    GPTQ.fasterquant(actorder=True, static_groups=True):
      per-channel scales from the whole row, dead columns zeroed, then -- grouped -- EVERY group's scale from the unswept weight in one
      launch (ops.group_scales), then the columns of W and H permuted by falling diag(H) (a stable sort: reproducible; it differs from the
      reference's unstable one only in the order of exactly equal entries), damping and the Cholesky chain on the permuted H, the sweep,
      and the result un-permuted.
    A block of the permuted order holds columns of many groups, so the grouped sweep is ops.gptq_block_cols under
    gidx = perm[i1:i2] // 128.  The groups stay contiguous: `scales` comes back [N, K / 128] in natural order and packs as ever.
    `perm`: the sweep order to use instead of the argsort (a permutation of range(K)); the result carries the order used.
    Grouped act_order without static_groups is refused: the groups would follow the permutation, which QuantLinear.pack cannot hold.
    static_groups has no effect per-channel (as in the reference); with neither switch this is gptq_quantize.  trace, fused, timers: as
    gptq_quantize; the timers also see "group_scales" and "permute" (the gathers)."""
    name = "gptq_quantize_ordered"
    if group_size not in (-1, BLOCK):
        raise NotImplementedError(f"{name}: only group_size -1 and 128 are supported")
    grouped = group_size == BLOCK
    if grouped and act_order and not static_groups:
        raise NotImplementedError(f"{name}: act_order with groups needs static_groups=True (moving groups follow the permutation, which "
                                  "QuantLinear.pack cannot hold)")
    if W.dim() != 2 or not W.is_cuda:
        raise RuntimeError(f"{name}: W must be a matrix on the GPU (there is no CPU path)")
    if not act_order and not (grouped and static_groups):
        return gptq_quantize(W, H, group_size, mse=mse, percdamp=percdamp, fused=fused, trace=trace, timers=timers)
    N, K = W.shape
    if H.shape != (K, K) or H.dtype != torch.float32 or H.device != W.device:
        raise RuntimeError(f"{name}: H must be float32 [{K}, {K}] on W's device")
    if K % 64 or (grouped and K % BLOCK):
        raise RuntimeError(f"{name}: K={K} must be a multiple of 64 (of 128 when grouped): QuantLinear's admission rule")
    if perm is not None:
        if not act_order:
            raise RuntimeError(f"{name}: perm is the order of act_order=True")
        if not isinstance(perm, torch.Tensor) or perm.dim() != 1 or perm.numel() != K or perm.is_floating_point():
            raise RuntimeError(f"{name}: perm must be an integer tensor [{K}]")
        perm = perm.to(device=W.device, dtype=torch.int64)
        if not torch.equal(torch.sort(perm).values, torch.arange(K, device=W.device)):  # (one read on the host: a bad index would fault)
            raise RuntimeError(f"{name}: perm is not a permutation of range({K})")
    section = timers.section if timers is not None else _no_section

    Wf = W.float().clone()
    with section("scales"):
        scale = None if grouped else ops.weight_scales(Wf, False, mse)
    H = H.clone()
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    Wf[:, dead] = 0
    S = None
    if grouped:
        with section("group_scales"):
            S = ops.group_scales(Wf, mse)
    invperm = None
    if act_order:
        with section("permute"):
            if perm is None:
                perm = torch.argsort(torch.diag(H), descending=True, stable=True)
            Wf = Wf[:, perm]
            H = H[perm][:, perm]
            invperm = torch.argsort(perm)
    if grouped:
        order = perm if act_order else torch.arange(K, device=W.device)
        gidx_all = (order // BLOCK).to(torch.int32)
    with section("cholesky"):
        Hinv = _upper_factor(H, percdamp)
    Q = torch.empty_like(Wf)
    Err1_buf = torch.empty((N, BLOCK), dtype=torch.float32, device=W.device)
    loss = torch.zeros((), dtype=torch.float32, device=W.device)
    blocks = []
    for i1 in range(0, K, BLOCK):
        i2 = min(i1 + BLOCK, K)
        W1, Hinv1 = Wf[:, i1:i2], Hinv[i1:i2, i1:i2]
        gidx = gidx_all[i1:i2] if grouped else None
        with section("sweep"):
            if fused and grouped:
                Q1, Err1 = ops.gptq_block_cols(W1, Hinv1, S, gidx, out=(Q[:, i1:i2], Err1_buf[:, :i2 - i1]))
            elif fused:
                Q1, Err1 = ops.gptq_block(W1, Hinv1, scale, False, out=(Q[:, i1:i2], Err1_buf[:, :i2 - i1]))
            else:
                Q1, Err1 = _block_cols_composed(W1, Hinv1, S[:, gidx.long()]) if grouped else _block_composed(W1, Hinv1, scale, False)
                Q[:, i1:i2] = Q1
        loss += (Err1 * Err1).sum() / 2
        if trace:
            blocks.append(BlockTrace(i1, W1.clone(), Q1.clone(), Err1.clone(), S[:, gidx.long()] if grouped else scale.clone()))
        if i2 < K:
            with section("gemm"):
                Wf[:, i2:] -= Err1.matmul(Hinv[i1:i2, i2:])
    if act_order:
        with section("permute"):
            Q = Q[:, invperm]
    weight = Q.to(W.dtype)
    s_extra = _s_extra(weight) if grouped else None
    return GPTQResult(weight, S if grouped else scale, s_extra, float(loss), blocks if trace else None, Hinv if trace else None,
                      perm if act_order else None)


@torch.no_grad()
def round_to_nearest(W: torch.Tensor, scales: torch.Tensor, grouped: bool) -> GPTQResult:
    """`W` [N, K] rounded to the nearest code under given scales ([N, 1] per-channel, [N, K / 128] grouped), with no error feedback: the
    yardstick GPTQ is measured against"""
    s = scales.repeat_interleave(BLOCK, dim=1) if grouped else scales
    weight = _quantise(W.float(), s, grouped).to(W.dtype)
    s_extra = _s_extra(weight) if grouped else None
    return GPTQResult(weight, scales, s_extra, 0.0)


class _NoSection:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _no_section(name):
    return _NoSection()
