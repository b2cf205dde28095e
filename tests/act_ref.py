"""Reference restatement of the decoder-block activation quantisers (include/qqq_amd_act.h) in numpy, and torch-side helpers the tests
share.  Formulas as the modules they replace compute them on fp16 inputs:
    LlamaRMSNorm (transformers):  h = fp16(residual + x);  n = fp16(float(h) * rsqrt(mean(float(h)^2) + eps));  y = fp16(float(w) * float(n))
    F.silu(g) * u:                s = fp16(g / (1 + exp(-g)));  y = fp16(float(s) * float(u))
    per-token quantisation (QuantLinear.dynamic_quant as the fused kernel evaluates it):
        s1 = float(fp16(amax * f32(1/127))),  q = clamp(rint(f32(y) / s1), -128, 127),  an all-zero row -> 0 codes, scale 0
"""
import numpy as np

F16, F32 = np.float16, np.float32


def quant_rows(y):
    """(int8 codes [m, k], f32 scales [m, 1]) of an fp16 [m, k] array."""
    y32 = np.asarray(y, F16).astype(F32)
    amax = np.abs(y32).max(axis=1, keepdims=True)
    s1 = (amax * F32(1.0 / 127.0)).astype(F32).astype(F16).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(s1 > 0, np.rint(y32 / np.where(s1 > 0, s1, F32(1))), F32(0))
    return np.clip(q, -128, 127).astype(np.int8), s1


def rmsnorm(x, w, eps, residual=None):
    """(y fp16, h fp16): LlamaRMSNorm of h = fp16(residual + x) (h = x without a residual)."""
    x = np.asarray(x, F16)
    h = x if residual is None else (np.asarray(residual, F16).astype(F32) + x.astype(F32)).astype(F16)
    h32 = h.astype(F32)
    var = (h32.astype(np.float64) ** 2).mean(axis=1, keepdims=True).astype(F32)
    n = (h32 * (F32(1) / np.sqrt(var + F32(eps), dtype=F32))).astype(F16)
    y = (np.asarray(w, F16).astype(F32) * n.astype(F32)).astype(F16)
    return y, h


def silu_mul(g, u):
    g32 = np.asarray(g, F16).astype(F32)
    with np.errstate(over="ignore"):
        s = (g32 / (F32(1) + np.exp(-g32, dtype=F32))).astype(F16)
    return (s.astype(F32) * np.asarray(u, F16).astype(F32)).astype(F16)


# ---- torch helpers (any device) ----

def ordered(t):
    """fp16 bits -> integers that are consecutive for consecutive fp16 values (+0 and -0 both 0)."""
    import torch

    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def from_ordered(o):
    import torch

    v = torch.where(o < 0, (-o) | 0x8000, o)
    return torch.where(v >= 0x8000, v - 0x10000, v).to(torch.int16).view(torch.float16)


def ulp_diff(a, b):
    """elementwise distance in fp16 ulps (two infinities of the same sign: 0)."""
    return (ordered(a) - ordered(b)).abs()


def torch_rmsnorm(x, w, eps, residual=None):
    """LlamaRMSNorm.forward of transformers on an fp16 tensor, as torch evaluates it; returns (y, n, h)."""
    import torch

    h = x if residual is None else residual + x
    hs = h.to(torch.float32)
    var = hs.pow(2).mean(-1, keepdim=True)
    n = (hs * torch.rsqrt(var + eps)).to(torch.float16)
    return w * n, n, h


def torch_silu_mul(g, u):
    import torch.nn.functional as F

    return F.silu(g) * u
