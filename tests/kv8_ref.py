"""Reference pieces of the int8 KV cache tests: the head-row quantiser as a torch expression, the exact dequantisation, a float64 attention."""
import torch


def quant_rows(x):
    """dynamic_quant of every last-dim row as a torch expression: (int8 codes x.shape, f32 scales x.shape[:-1]).  The scale is
    float(fp16(amax * (1/127))); an all-zero row (and one whose scale rounds to zero) gives zero codes."""
    xf = x.float()
    s = (xf.abs().amax(-1, keepdim=True) * (1.0 / 127.0)).half().float()
    q = torch.where(s > 0, torch.clamp(torch.round(xf / s.clamp_min(1e-30)), -128, 127), torch.zeros_like(xf))
    return q.to(torch.int8), s.squeeze(-1)


def quant_rows_op(x):
    """The same through the project's own op on the GPU: (codes, scales) of fp16 x [..., d]"""
    from qqq_amd import ops

    codes, s = ops.dynamic_quant(x.contiguous())
    return codes, s.squeeze(-1).contiguous()


def dequant64(codes, scales):
    """code * scale in float64: exact (8-bit integer times a 24-bit significand)"""
    return codes.double() * scales.double()[..., None]


def attention64(q, k64, v64, pos, scale):
    """float64 attention of q fp16 [b, h, 1, d] over keys 0 ... pos[bi] of k64 / v64 [b, kvh, cap, d] -> [b, h, d]"""
    b, h, _, d = q.shape
    kvh = k64.shape[1]
    out = torch.empty((b, h, d), dtype=torch.float64, device=q.device)
    for bi in range(b):
        p = int(pos[bi])
        k = k64[bi, :, :p + 1].repeat_interleave(h // kvh, 0)
        v = v64[bi, :, :p + 1].repeat_interleave(h // kvh, 0)
        s = torch.einsum("hd,hkd->hk", q[bi, :, 0].double(), k) * scale
        out[bi] = torch.einsum("hk,hkd->hd", torch.softmax(s, -1), v)
    return out
