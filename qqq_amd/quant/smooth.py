"""Smoothing before GPTQ: the reference's outlier migration (QQQ/smooth, examples/quant_model.py --smooth True) over state dicts.  Per
decoder layer four per-channel scale vectors s (qkv, o, gate_up, down) move activation outliers into the weights: X / s, W * s.  The
search of a scale runs a module function (fp16 matmuls; for qkv RoPE, repeat_kv, the additive causal mask and an f32 softmax) on
fake-quantised operands for every candidate and keeps the candidate of least loss; the two fake-quantisations per candidate are ONE launch
each (ops.fake_quant_rows) where the reference composes about fourteen torch launches (fake_quant_torch, kept as fused=False: the
benchmark's baseline and a cross-check with the same bits).  transformers is not imported.

Out of scope: token-wise clipping (the reference's QuantileObserver), padded batches and observation masks (sequences are of equal
length), bf16 / f32 models, SDPA inside the search."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from ..attention import _config_rope, rope_inv_freq, rope_tables
from . import ops

KINDS = ("qkv", "o_proj", "up_and_gate", "down_proj")
METHODS = ("os+", "awq", "sq")
EPS = 1.1920929e-07  # torch.finfo(torch.float32).eps; as fp16 the subnormal 2^-23


def fake_quant_torch(x: torch.Tensor, col_scale, bits: int, group: int = 0, divide: bool = False) -> torch.Tensor:
    """ops.fake_quant_rows composed from torch calls in the reference's order (MigratorBase.quantize: MinMaxObserver, calculate_qparams,
    fake_quantize_per_channel_affine with its round_ste and integer zero point) -- the same bits, about fourteen launches.  Any device."""
    qmax = 2 ** (bits - 1) - 1
    t = x if col_scale is None else (x / col_scale if divide else x * col_scale)
    X = t.reshape(-1, group) if group else t
    mn, mx = torch.aminmax(X, dim=1)
    mn_neg = torch.min(mn, torch.zeros_like(mn))
    mx_pos = torch.max(mx, torch.zeros_like(mx))
    mx_pos = torch.max(-mn_neg, mx_pos)
    scale = mx_pos / (float(qmax + qmax) / 2)
    scale = torch.max(scale, torch.tensor([EPS], dtype=torch.float32, device=x.device).to(x.dtype)).reshape(-1, 1)
    zp = torch.zeros(scale.shape, dtype=torch.int, device=x.device)
    v = X / scale
    x_int = ((v.round() - v) + v) + zp
    x_q = torch.clamp(x_int, -qmax, qmax)
    return ((x_q - zp) * scale).reshape(x.shape)


def _fq(x2d, col_scale, bits, group, divide, fused, out=None):
    if fused:
        return ops.fake_quant_rows(x2d, col_scale, bits, group, divide, out=out)
    return fake_quant_torch(x2d, col_scale, bits, group, divide)


def _rotate_half(x):
    half = x.shape[-1] // 2
    return torch.cat((-x[..., half:], x[..., :half]), dim=-1)


def causal_mask(length: int, device, dtype=torch.float16) -> torch.Tensor:
    """the additive causal mask [1, 1, length, length] the reference's model hands the search: 0 on and below the diagonal, finfo.min above"""
    return torch.full((length, length), torch.finfo(dtype).min, dtype=dtype, device=device).triu(1)[None, None]


def attention_extra(config, length: int, device, bias=None, q_norm=None, k_norm=None) -> dict:
    """the `extra` of kind "qkv" for a (duck-typed) Llama / Qwen2 / Qwen3 config: head counts, RoPE tables [length, head_dim], the causal
    mask; `q_norm`, `k_norm`: a Qwen3 layer's per-head norm weights [head_dim] (applied to q and k before RoPE, eps = rms_norm_eps)"""
    heads = config.num_attention_heads
    kv_heads = getattr(config, "num_key_value_heads", None) or heads
    head_dim = getattr(config, "head_dim", None) or config.hidden_size // heads
    theta, rope = _config_rope(config)
    inv_freq, scaling = rope_inv_freq(head_dim, theta, rope)
    cos, sin = rope_tables(inv_freq, scaling, length, device)
    return {"num_heads": heads, "num_key_value_heads": kv_heads, "head_dim": head_dim, "cos": cos[:length], "sin": sin[:length],
            "mask": causal_mask(length, device), "bias": bias, "q_norm": q_norm, "k_norm": k_norm, "eps": config.rms_norm_eps}


def _attend(q, k, v, extra):
    # q [B, heads, N, d], k and v [B, kv_heads, N, d] -> [B, N, heads * d]; the reference's explicit composition, no SDPA
    B, _, N, d = q.shape
    cos, sin = extra["cos"][None, None], extra["sin"][None, None]
    if extra.get("q_norm") is not None:  # Qwen3: RMSNorm over head_dim between the projections and RoPE
        q, k = _rms_norm(q, extra["q_norm"], extra["eps"]), _rms_norm(k, extra["k_norm"], extra["eps"])
    q = q * cos + _rotate_half(q) * sin
    k = k * cos + _rotate_half(k) * sin
    rep = extra["num_heads"] // extra["num_key_value_heads"]
    if rep > 1:  # repeat_kv
        k = k[:, :, None].expand(B, k.shape[1], rep, N, d).reshape(B, -1, N, d)
        v = v[:, :, None].expand(B, v.shape[1], rep, N, d).reshape(B, -1, N, d)
    attn = (q / math.sqrt(d)) @ k.transpose(-2, -1)
    attn = attn + extra["mask"]
    attn = torch.max(attn, torch.tensor(torch.finfo(q.dtype).min, device=q.device))
    attn = attn.softmax(dim=-1, dtype=torch.float32).to(q.dtype)
    return (attn @ v).transpose(1, 2).reshape(B, N, -1)


def module_output(kind: str, x: torch.Tensor, weight: torch.Tensor, extra: Optional[dict] = None) -> torch.Tensor:
    """the reference's module functions (MigratorBase.get_output): x fp16 [B, N, K], weight fp16 [rows, K] -> f32 [B * N, features]"""
    B, N, _ = x.shape
    if kind == "qkv":
        d, heads, kv_heads = extra["head_dim"], extra["num_heads"], extra["num_key_value_heads"]
        qkv = torch.matmul(x, weight.T)
        if extra.get("bias") is not None:
            qkv = qkv + extra["bias"]
        sz_q, sz_kv = heads * d, kv_heads * d
        q = qkv[:, :, :sz_q].view(B, N, heads, d).transpose(1, 2)
        k = qkv[:, :, sz_q:sz_q + sz_kv].view(B, N, kv_heads, d).transpose(1, 2)
        v = qkv[:, :, sz_q + sz_kv:].view(B, N, kv_heads, d).transpose(1, 2)
        out = _attend(q, k, v, extra)
    elif kind in ("o_proj", "down_proj"):
        out = torch.matmul(x, weight.T)
    elif kind == "up_and_gate":
        C = weight.shape[0]
        out = torch.matmul(x, weight.T).reshape(B, N, 2, C // 2).permute(2, 0, 1, 3)
        out = F.silu(out[0]) * out[1]
    else:
        raise RuntimeError(f"module_output: kind must be one of {KINDS}, got {kind!r}")
    return out.reshape(B * N, -1).to(torch.float32)


def loss_fx(pred: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
    return (pred - tgt).abs().pow(2.0).sum(-1).mean()


def range_scale(cmn: torch.Tensor, cmx: torch.Tensor, st: float) -> torch.Tensor:
    """the scale of clipping range (-st, st), in fp16 (MigratorBase.cac_scale): channels whose extremes pass the range are scaled back to it"""
    one = torch.tensor(1.0, dtype=cmx.dtype, device=cmx.device)
    mx_r = torch.tensor(st, dtype=cmx.dtype, device=cmx.device)
    mn_r = torch.tensor(-st, dtype=cmx.dtype, device=cmx.device)
    return torch.max(torch.where(cmx > mx_r, cmx / mx_r, one), torch.where(cmn < mn_r, cmn / mn_r, one))


def candidate_ranges(amn: float, amx: float) -> list:
    """the clipping ranges Migrator1DRangeSearch walks, in Python floats: from max(-amn, amx) down to 0.1 in max(100, int(amx / 0.5)) steps"""
    num = max(100, int(amx / 0.5))
    bounds = (0.1, max(-amn, amx))
    step = (bounds[1] - bounds[0]) / num
    st, out = bounds[1], []
    while st >= bounds[0]:
        out.append(st)
        st -= step
    return out


def earliest_minimum(losses) -> int:
    """the index the reference's `best_loss is None or best_loss > loss` walk ends on"""
    best = 0
    for i, v in enumerate(losses):
        if losses[best] > v:
            best = i
    return best


@torch.no_grad()
def migration_scale(x: torch.Tensor, weight: torch.Tensor, kind: str, group_size: int, method: str = "os+", extra: Optional[dict] = None,
                    fused: bool = True, trace: Optional[dict] = None) -> torch.Tensor:
    """The migration scale (fp16 [K]) of one module: `x` fp16 [B, N, K] is its input, `weight` fp16 [rows, K] the concatenation the
    reference passes (q|k|v, o, gate|up, down), `kind` one of "qkv", "o_proj", "up_and_gate", "down_proj" (`extra`: attention_extra(...)
    for "qkv"), `group_size` -1 (a 4-bit scale per weight row) or 128.
    method "os+" (default): Migrator1DRangeSearch -- every clipping range of candidate_ranges() gives a scale (range_scale); the module runs on
    fake_quant(x / s, 8 bits per token) and fake_quant(W * s, 4 bits); the earliest strictly least loss against the float output wins.
    "awq": the 20-point ratio grid over mean |x| (its activation is quantised as the reference does without a clipping range: per group
    of 128 with group_size 128, per batch element otherwise).  "sq": the closed form with alpha 0.5, no search.
    fused=False composes the fake-quantisations from torch calls (fake_quant_torch): the same bits, the reference's launch count.
    `trace`: a dict that receives "ranges" (os+) or "ratios" (awq), "losses" (Python floats of the f32 losses) and "best" (the index)."""
    if kind not in KINDS:
        raise RuntimeError(f"migration_scale: kind must be one of {KINDS}, got {kind!r}")
    if method not in METHODS:
        raise RuntimeError(f"migration_scale: method must be one of {METHODS}, got {method!r}")
    if group_size not in (-1, 128):
        raise RuntimeError(f"migration_scale: group_size must be -1 or 128, got {group_size!r}")
    if not (isinstance(x, torch.Tensor) and x.dim() == 3 and x.dtype == torch.float16 and isinstance(weight, torch.Tensor)
            and weight.dim() == 2 and weight.dtype == torch.float16 and weight.shape[1] == x.shape[2]):
        raise RuntimeError("migration_scale: x must be float16 [B, N, K] and weight float16 [rows, K]")
    B, N, K = x.shape
    group = 0 if group_size == -1 else group_size
    cmx = x.max(0)[0].max(0)[0]
    cmn = x.min(0)[0].min(0)[0]
    if method == "sq":
        act = torch.max(cmx.abs(), cmn.abs())
        wsc = weight.abs().max(dim=0)[0].clamp(min=1e-5)
        return (act.pow(0.5) / wsc.pow(0.5)).clamp(min=1e-5).to(x.dtype)
    tgt = module_output(kind, x, weight, extra)
    x2 = x.reshape(B * N, K)
    weight = weight.contiguous()
    qx, qw = (torch.empty_like(x2), torch.empty_like(weight)) if fused else (None, None)

    def loss_of(scale, per_token):
        if per_token:
            a = _fq(x2, scale, 8, 0, True, fused, out=qx)
        elif group:  # no clipping range: the reference reshapes the activation like the weight, to groups of 128
            a = _fq(x2, scale, 8, group, True, fused, out=qx)
        else:  # ... and otherwise takes one scale per batch element: the scaled activation is formed first, a row is a whole element
            a = _fq((x / scale).reshape(B, N * K), None, 8, 0, True, fused)
        w = _fq(weight, scale, 4, group, False, fused, out=qw)
        return loss_fx(module_output(kind, a.reshape(B, N, K), w, extra), tgt)

    if method == "os+":
        amx = max(x.max().item(), 0.0)
        amn = min(x.min().item(), 0.0)
        ranges = candidate_ranges(amn, amx)
        if not ranges:  # an input inside (-0.1, 0.1): the reference's walk never starts and keeps the whole range
            if trace is not None:
                trace.update(ranges=[], losses=[], best=None)
            return range_scale(cmn, cmx, max(-amn, amx))
        losses = torch.stack([loss_of(range_scale(cmn, cmx, st), True) for st in ranges]).tolist()
        best = earliest_minimum(losses)
        if trace is not None:
            trace.update(ranges=ranges, losses=losses, best=best)
        return range_scale(cmn, cmx, ranges[best])
    # awq
    x_max = x.abs().view(-1, K).mean(0)
    ratios = [cnt / 20 for cnt in range(20)]
    scales = []
    for ratio in ratios:
        s = x_max.pow(ratio).clamp(min=1e-4).view(-1)
        scales.append(s / (s.max() * s.min()).sqrt())
    losses = torch.stack([loss_of(s, False) for s in scales]).tolist()
    best, least = -1, float("inf")
    for i, v in enumerate(losses):
        if v < least:
            best, least = i, v
    if best < 0:
        raise RuntimeError(f"migration_scale: no awq candidate has a finite loss: {losses}")
    if trace is not None:
        trace.update(ratios=ratios, losses=losses, best=best)
    return scales[best]


def _rms_norm(x, weight, eps):
    h = x.float()
    h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)
    return weight * h.to(x.dtype)


def _layer_weights(state_dict, i, dev):
    prefix = f"model.layers.{i}."
    return {k[len(prefix):]: v.to(dev).half() for k, v in state_dict.items() if k.startswith(prefix)}


@torch.no_grad()
def smooth_scales(state_dict: dict, config, calib_ids: torch.Tensor, group_size: int, method: str = "os+", batch_size: int = 8,
                  device=None, fused: bool = True) -> list:
    """The reference's scale_list for an fp16 Llama / Qwen2 state dict: four fp16 [K] vectors per layer in its order (qkv, o, gate_up,
    down), on `device`.  Only the first `batch_size` sequences of `calib_ids` [samples, seqlen] are used, as ONE batch (the reference
    calibrates on its first batch alone).  Per layer: norm, search, h /= s and W *= s in fp16, then the module runs with its input
    fake-quantised per token to 8 bits and its weights to 4 (ops.fake_quant_rows with col_scale=None), so every later search sees the
    quantised model's activations."""
    dev = torch.device(device if device is not None else "cuda:0")
    ids = torch.as_tensor(calib_ids, dtype=torch.int64, device=dev)
    if ids.dim() != 2:
        raise RuntimeError("smooth_scales: calib_ids must be [samples, seqlen] token ids")
    if group_size not in (-1, 128):
        raise RuntimeError(f"smooth_scales: group_size must be -1 or 128, got {group_size!r}")
    ids = ids[:batch_size]
    group = 0 if group_size == -1 else group_size
    x = F.embedding(ids, state_dict["model.embed_tokens.weight"].to(dev).half())
    B, N, _ = x.shape
    eps = config.rms_norm_eps

    def fq_act(h):
        return _fq(h.reshape(B * N, -1), None, 8, 0, True, fused).reshape(B, N, -1)

    def fq_w(w):
        return _fq(w.contiguous(), None, 4, group, False, fused)

    scale_list = []
    for i in range(config.num_hidden_layers):
        w = _layer_weights(state_dict, i, dev)
        names = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")
        biases = [w.get(n + ".bias") for n in names]
        bias = torch.cat(biases) if all(b is not None for b in biases) else None
        extra = attention_extra(config, N, dev, bias, w.get("self_attn.q_norm.weight"), w.get("self_attn.k_norm.weight"))
        # q | k | v
        h = _rms_norm(x, w["input_layernorm.weight"], eps)
        wqkv = torch.cat([w[n + ".weight"] for n in names])
        s = migration_scale(h, wqkv, "qkv", group_size, method, extra, fused)
        scale_list.append(s)
        h = fq_act(h / s)
        qkv = torch.matmul(h, fq_w(wqkv * s).T)
        if bias is not None:
            qkv = qkv + bias
        d, heads, kv_heads = extra["head_dim"], extra["num_heads"], extra["num_key_value_heads"]
        q = qkv[:, :, :heads * d].view(B, N, heads, d).transpose(1, 2)
        k = qkv[:, :, heads * d:(heads + kv_heads) * d].view(B, N, kv_heads, d).transpose(1, 2)
        v = qkv[:, :, (heads + kv_heads) * d:].view(B, N, kv_heads, d).transpose(1, 2)
        a = _attend(q, k, v, extra)
        # o
        wo = w["self_attn.o_proj.weight"]
        s = migration_scale(a, wo, "o_proj", group_size, method, None, fused)
        scale_list.append(s)
        o = torch.matmul(fq_act(a / s), fq_w(wo * s).T)
        if w.get("self_attn.o_proj.bias") is not None:
            o = o + w["self_attn.o_proj.bias"]
        x = x + o
        # gate | up
        h = _rms_norm(x, w["post_attention_layernorm.weight"], eps)
        wgu = torch.cat([w["mlp.gate_proj.weight"], w["mlp.up_proj.weight"]])
        s = migration_scale(h, wgu, "up_and_gate", group_size, method, None, fused)
        scale_list.append(s)
        h = fq_act(h / s)
        inter = w["mlp.gate_proj.weight"].shape[0]
        m = F.silu(torch.matmul(h, fq_w(wgu[:inter] * s).T)) * torch.matmul(h, fq_w(wgu[inter:] * s).T)
        # down
        wd = w["mlp.down_proj.weight"]
        s = migration_scale(m, wd, "down_proj", group_size, method, None, fused)
        scale_list.append(s)
        x = x + torch.matmul(fq_act(m / s), fq_w(wd * s).T)
    return scale_list


@torch.no_grad()
def apply_smooth(state_dict: dict, config, scale_list: list) -> dict:
    """A new state dict with the scales folded in, in fp16: the reference's export_smoothed_model for Llama and Qwen2.  Per layer and in
    the list's order: input norm /= s, q k v *= s;  o *= s with v's rows (and v's bias) /= s -- only when num_key_value_heads ==
    num_attention_heads, the scale is consumed from the list either way;  post-attention norm /= s, gate up *= s;  down *= s with up's
    rows /= s.  Every other tensor is passed through."""
    layers = config.num_hidden_layers
    if not isinstance(scale_list, (list, tuple)) or len(scale_list) != 4 * layers:
        raise RuntimeError(f"apply_smooth: scale_list must hold 4 * {layers} vectors, got "
                           f"{len(scale_list) if isinstance(scale_list, (list, tuple)) else type(scale_list).__name__}")
    heads = config.num_attention_heads
    kv_heads = getattr(config, "num_key_value_heads", None) or heads
    out = dict(state_dict)

    def get(key):
        t = state_dict[key]
        if t.dtype != torch.float16:
            raise RuntimeError(f"apply_smooth: {key} is {str(t.dtype).replace('torch.', '')}; smoothing is done in float16")
        return t

    def sc(j, like, n):
        s = scale_list[j]
        if not isinstance(s, torch.Tensor) or s.dtype != torch.float16 or s.dim() != 1 or s.numel() != n:
            raise RuntimeError(f"apply_smooth: scale {j} must be float16 [{n}]")
        return s.to(like.device)

    for i in range(layers):
        p = f"model.layers.{i}."
        ln = get(p + "input_layernorm.weight")
        s = sc(4 * i, ln, ln.numel())
        out[p + "input_layernorm.weight"] = ln / s
        for n in ("q_proj", "k_proj", "v_proj"):
            out[p + f"self_attn.{n}.weight"] = get(p + f"self_attn.{n}.weight") * s
        wo = get(p + "self_attn.o_proj.weight")
        s = sc(4 * i + 1, wo, wo.shape[1])
        if kv_heads == heads:
            out[p + "self_attn.o_proj.weight"] = wo * s
            out[p + "self_attn.v_proj.weight"] = out[p + "self_attn.v_proj.weight"] / s.reshape(-1, 1)
            if p + "self_attn.v_proj.bias" in state_dict:
                out[p + "self_attn.v_proj.bias"] = get(p + "self_attn.v_proj.bias") / s
        ln = get(p + "post_attention_layernorm.weight")
        s = sc(4 * i + 2, ln, ln.numel())
        out[p + "post_attention_layernorm.weight"] = ln / s
        for n in ("gate_proj", "up_proj"):
            out[p + f"mlp.{n}.weight"] = get(p + f"mlp.{n}.weight") * s
        wd = get(p + "mlp.down_proj.weight")
        s = sc(4 * i + 3, wd, wd.shape[1])
        out[p + "mlp.down_proj.weight"] = wd * s
        out[p + "mlp.up_proj.weight"] = out[p + "mlp.up_proj.weight"] / s.reshape(-1, 1)
    return out


@torch.no_grad()
def smooth_model(state_dict: dict, config, calib_ids: torch.Tensor, group_size: int, method: str = "os+", batch_size: int = 8,
                 device=None, fused: bool = True):
    """smooth_scales, then apply_smooth -> (the smoothed state dict, the scale_list)"""
    scale_list = smooth_scales(state_dict, config, calib_ids, group_size, method, batch_size, device, fused)
    return apply_smooth(state_dict, config, scale_list), scale_list
