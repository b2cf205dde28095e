"""Torch restatement of transformers' rotary embedding and SDPA attention (models/llama/modeling_llama.py, integrations/sdpa_attention.py),
the reference the attention tests hold rope_qkv and the attention / decoder-layer modules to.

    rotate_half(x) = cat(-x[..., d/2:], x[..., :d/2]);   apply_rotary(x) = x * cos + rotate_half(x) * sin   (fp16 tensor ops: each op is
    evaluated in fp32 and rounded to fp16, so out = fp16(fp16(x * cos) + fp16(rotate_half(x) * sin)))
    sdpa(q, k, v, start): F.scaled_dot_product_attention over keys 0 ... start+s-1, causal with the diagonal at the bottom right
"""
import torch
import torch.nn.functional as F


def rotate_half(x):
    x1 = x[..., : x.shape[-1] // 2]
    x2 = x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def apply_rotary(x, cos, sin, unsqueeze_dim=1):
    """apply_rotary_pos_emb for one tensor: x [b, heads, s, d], cos / sin [b, s, d] (unsqueeze_dim=1) or already broadcastable (None)."""
    if unsqueeze_dim is not None:
        cos, sin = cos.unsqueeze(unsqueeze_dim), sin.unsqueeze(unsqueeze_dim)
    return (x * cos) + (rotate_half(x) * sin)


def rope_rows(x, heads, cos, sin, pos):
    """apply_rotary on token rows: x [m, heads*d] -> [m, heads, d], each token rotated by the table rows at its position pos [m]."""
    m = x.shape[0]
    xv = x.reshape(m, heads, -1)
    return apply_rotary(xv, cos[pos], sin[pos], unsqueeze_dim=1)


def causal_mask(s, kv_len, device):
    """bool [s, kv_len]: query i (at position kv_len - s + i) sees keys 0 ... kv_len - s + i."""
    return torch.ones((s, kv_len), dtype=torch.bool, device=device).tril(diagonal=kv_len - s)


def sdpa(q, k, v, start, scaling, num_kv_heads):
    """scaled_dot_product_attention of q [b, h, s, d] over k / v [b, kvh, >= start+s, d] as the attention module calls it -> [b, s, h*d]."""
    b, h, s, d = q.shape
    k, v = k[:, :, :start + s], v[:, :, :start + s]
    mask = causal_mask(s, start + s, q.device) if (s > 1 and start > 0) else None
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, is_causal=(s > 1 and start == 0), scale=scaling,
                                       enable_gqa=h != num_kv_heads)
    return o.transpose(1, 2).reshape(b, s, h * d)


def repeat_kv(x, n_rep):
    b, kvh, s, d = x.shape
    return x[:, :, None].expand(b, kvh, n_rep, s, d).reshape(b, kvh * n_rep, s, d)


def attention(x, w, heads, kv_heads, cos, sin, start=0, k_past=None, v_past=None):
    """transformers' LlamaAttention on x [b, s, hidden] in plain torch (eager softmax, repeat_kv), for tokens at start ... start+s-1.
    w: {q, k, v, o: (weight [out, in], bias or None)}; cos / sin: tables [>= start+s, d].  k_past / v_past [b, kvh, start, d] or None.
    Returns (out [b, s, hidden], k [b, kvh, start+s, d], v)."""
    b, s, _ = x.shape
    lin = lambda name, t: F.linear(t, *w[name])
    q = lin("q", x).view(b, s, heads, -1).transpose(1, 2)
    k = lin("k", x).view(b, s, kv_heads, -1).transpose(1, 2)
    v = lin("v", x).view(b, s, kv_heads, -1).transpose(1, 2)
    d = q.shape[-1]
    c, sn = cos[start:start + s][None], sin[start:start + s][None]
    q, k = apply_rotary(q, c, sn), apply_rotary(k, c, sn)
    if k_past is not None:
        k, v = torch.cat((k_past, k), 2), torch.cat((v_past, v), 2)
    kr, vr = repeat_kv(k, heads // kv_heads), repeat_kv(v, heads // kv_heads)
    scores = (q @ kr.transpose(2, 3)) * d ** -0.5
    scores = scores.masked_fill(~causal_mask(s, start + s, x.device), float("-inf"))
    o = torch.softmax(scores.float(), dim=-1).to(q.dtype) @ vr
    return lin("o", o.transpose(1, 2).reshape(b, s, -1)), k, v
