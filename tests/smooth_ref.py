"""CPU restatement of the smoothing stage (QQQ/smooth/migration): fake_quant_rows in numpy, one f32 operation rounded to fp16 per line as
qqq_amd_fakequant.h states it, and the three searches with the module functions in torch on the CPU.  Nothing of qqq_amd is imported."""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS16 = np.float16(1.1920929e-07)  # 2^-23


def _h(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16)


def fake_quant_rows(x, col_scale, bits, group=0, divide=False):
    """x fp16 [rows, cols] (numpy), col_scale None or fp16 [cols] -> fp16 [rows, cols]"""
    x = np.asarray(x)
    assert x.dtype == np.float16 and x.ndim == 2
    qmax = np.float32(2 ** (bits - 1) - 1)
    with np.errstate(all="ignore"):
        if col_scale is None:
            t = x
        else:
            c = np.asarray(col_scale).astype(np.float32)[None, :]
            t = _h(x.astype(np.float32) / c) if divide else _h(x.astype(np.float32) * c)
        T = t.reshape(-1, group) if group else t
        mn = np.minimum(T.min(axis=1), np.float16(0))
        mx = np.maximum(T.max(axis=1), np.float16(0))
        a = np.maximum(-mn, mx)
        s = np.maximum(_h(a.astype(np.float32) / qmax), EPS16)[:, None].astype(np.float32)
        r = np.rint(_h(T.astype(np.float32) / s).astype(np.float32))  # half to even
        r = np.clip(r, -qmax, qmax) + np.float32(0)  # -0 -> +0
        y = _h(r * s)
    return y.reshape(x.shape)


def fq_t(x2d: torch.Tensor, col_scale, bits, group=0, divide=False) -> torch.Tensor:
    c = None if col_scale is None else col_scale.numpy()
    return torch.from_numpy(fake_quant_rows(x2d.contiguous().numpy(), c, bits, group, divide))


def rope_tables(head_dim, length, theta=10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    freqs = (inv[None, :, None] @ torch.arange(length)[None, None, :].float()).transpose(1, 2)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().half()[0], emb.sin().half()[0]


def causal_mask(length):
    return torch.full((length, length), torch.finfo(torch.float16).min, dtype=torch.float16).triu(1)[None, None]


def make_extra(heads, kv_heads, head_dim, length, theta=10000.0):
    cos, sin = rope_tables(head_dim, length, theta)
    return {"num_heads": heads, "num_key_value_heads": kv_heads, "head_dim": head_dim, "cos": cos, "sin": sin, "mask": causal_mask(length)}


def _rot(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def module_output(kind, x, w, extra=None):
    B, N, _ = x.shape
    if kind == "qkv":
        d, nh, nkv = extra["head_dim"], extra["num_heads"], extra["num_key_value_heads"]
        qkv = torch.matmul(x, w.T)
        q = qkv[:, :, :nh * d].view(B, N, nh, d).transpose(1, 2)
        k = qkv[:, :, nh * d:(nh + nkv) * d].view(B, N, nkv, d).transpose(1, 2)
        v = qkv[:, :, (nh + nkv) * d:].view(B, N, nkv, d).transpose(1, 2)
        cos, sin = extra["cos"][None, None], extra["sin"][None, None]
        q, k = q * cos + _rot(q) * sin, k * cos + _rot(k) * sin
        rep = nh // nkv
        k = k[:, :, None].expand(B, nkv, rep, N, d).reshape(B, nh, N, d)
        v = v[:, :, None].expand(B, nkv, rep, N, d).reshape(B, nh, N, d)
        attn = (q / math.sqrt(d)) @ k.transpose(-2, -1) + extra["mask"]
        attn = torch.max(attn, torch.tensor(torch.finfo(torch.float16).min))
        attn = attn.softmax(dim=-1, dtype=torch.float32).half()
        out = (attn @ v).transpose(1, 2).reshape(B, N, -1)
    elif kind == "up_and_gate":
        o = torch.matmul(x, w.T).reshape(B, N, 2, w.shape[0] // 2).permute(2, 0, 1, 3)
        out = F.silu(o[0]) * o[1]
    else:
        out = torch.matmul(x, w.T)
    return out.reshape(B * N, -1).float()


def loss_fx(pred, tgt):
    return (pred - tgt).abs().pow(2.0).sum(-1).mean()


def range_scale(cmn, cmx, st):
    one = torch.tensor(1.0, dtype=torch.float16)
    hi, lo = torch.tensor(st, dtype=torch.float16), torch.tensor(-st, dtype=torch.float16)
    return torch.max(torch.where(cmx > hi, cmx / hi, one), torch.where(cmn < lo, cmn / lo, one))


def candidate_ranges(x):
    amx = max(x.max().item(), 0.0)
    amn = min(x.min().item(), 0.0)
    num = max(100, int(amx / 0.5))
    hi = max(-amn, amx)
    step = (hi - 0.1) / num
    st, out = hi, []
    while st >= 0.1:
        out.append(st)
        st -= step
    return out


def os_loss(x, w, kind, group, st, extra=None, tgt=None):
    """the loss of clipping range st, and the two fake-quantised operands"""
    B, N, K = x.shape
    cmx, cmn = x.max(0)[0].max(0)[0], x.min(0)[0].min(0)[0]
    s = range_scale(cmn, cmx, st)
    qx = fq_t(x.reshape(B * N, K), s, 8, 0, True)
    qw = fq_t(w, s, 4, group, False)
    if tgt is None:
        tgt = module_output(kind, x, w, extra)
    return loss_fx(module_output(kind, qx.reshape(B, N, K), qw, extra), tgt).item(), qx, qw


def search_os(x, w, kind, group, extra=None):
    """-> (scale fp16 [K], ranges, losses, best index)"""
    tgt = module_output(kind, x, w, extra)
    ranges = candidate_ranges(x)
    losses = [os_loss(x, w, kind, group, st, extra, tgt)[0] for st in ranges]
    best = 0
    for i, v in enumerate(losses):
        if losses[best] > v:
            best = i
    cmx, cmn = x.max(0)[0].max(0)[0], x.min(0)[0].min(0)[0]
    return range_scale(cmn, cmx, ranges[best]), ranges, losses, best


def search_awq(x, w, kind, group, extra=None):
    """-> (scale, ratios, losses, best index); the activation is quantised per group of 128, or per batch element with group 0"""
    B, N, K = x.shape
    tgt = module_output(kind, x, w, extra)
    x_max = x.abs().view(-1, K).mean(0)
    ratios, scales, losses = [c / 20 for c in range(20)], [], []
    for ratio in ratios:
        s = x_max.pow(ratio).clamp(min=1e-4).view(-1)
        s = s / (s.max() * s.min()).sqrt()
        if group:
            qx = fq_t(x.reshape(B * N, K), s, 8, group, True)
        else:
            qx = fq_t((x / s).reshape(B, N * K), None, 8, 0, True)
        qw = fq_t(w, s, 4, group, False)
        scales.append(s)
        losses.append(loss_fx(module_output(kind, qx.reshape(B, N, K), qw, extra), tgt).item())
    best = min(range(20), key=lambda i: (losses[i], i))
    return scales[best], ratios, losses, best


def search_sq(x, w):
    cmx, cmn = x.max(0)[0].max(0)[0], x.min(0)[0].min(0)[0]
    act = torch.max(cmx.abs(), cmn.abs())
    ws = w.abs().max(dim=0)[0].clamp(min=1e-5)
    return (act.pow(0.5) / ws.pow(0.5)).clamp(min=1e-5).half()


KINDS = ("qkv", "qkv_gqa", "o_proj", "up_and_gate", "down_proj")
HEADS, HEAD_DIM = 4, 64


def golden_case(g, kind, group):
    """(x, w, module kind, extra, the recorded case as a dict) of tests/golden/smooth_small.npz (gen_smooth_golden.py)"""
    x = torch.from_numpy(g[f"{kind}/x"])
    w = (torch.from_numpy(g[f"{kind}/w_code"].astype(np.float32)) / 128).half()
    extra = None
    if kind in ("qkv", "qkv_gqa"):
        extra = {"num_heads": HEADS, "num_key_value_heads": HEADS if kind == "qkv" else HEADS // 2, "head_dim": HEAD_DIM,
                 "cos": torch.from_numpy(g[f"{kind}/cos"]), "sin": torch.from_numpy(g[f"{kind}/sin"]), "mask": causal_mask(x.shape[1])}
    tag = f"{kind}_{'g128' if group else 'pc'}"
    rec = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(tag + "/") or k.startswith(kind + "/")}
    return x, w, "qkv" if kind == "qkv_gqa" else kind, extra, rec
