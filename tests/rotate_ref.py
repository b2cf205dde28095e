"""CPU restatement of the rotation op and flow in numpy f64 (qqq_amd/quant/include/qqq_amd_rotate.h, qqq_amd/quant/rotation.py): the
stages in the stated order, one divide, the two-step rounding.  The tests hold the HIP op to it bit for bit, and hold it to the fixture
recorded from the reference's own rotation (tests/golden/rotate_small.npz, gen_rotate_golden.py)."""
import numpy as np

RIGHT = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight")
FUSED_BY = {"input_layernorm.weight": ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"),
            "post_attention_layernorm.weight": ("mlp.gate_proj.weight", "mlp.up_proj.weight")}


def divisor(n):
    """(double)sqrtf((float)n)"""
    return np.float64(np.sqrt(np.float32(n)))


def to_dtype(v64, dtype):
    """f64 -> f32 -> dtype: torch's conversion of f64 to fp16 rounds twice"""
    return np.asarray(v64, np.float64).astype(np.float32).astype(dtype)


def wht_f64(v, n, sign=None):
    """every block of n consecutive entries of the last axis of the f64 array v: (v * sign) . H_n / d, stage by stage, in f64"""
    v = np.array(v, dtype=np.float64)
    shape = v.shape
    assert shape[-1] % n == 0 and n >= 1 and n & (n - 1) == 0
    v = v.reshape(-1, n)
    if sign is not None:
        v = v * np.asarray(sign).astype(np.float64)
    h = 1
    while h < n:
        w = v.reshape(-1, n // (2 * h), 2, h)
        a, b = w[:, :, 0, :].copy(), w[:, :, 1, :].copy()
        w[:, :, 0, :] = a + b  # i with (i & h) == 0
        w[:, :, 1, :] = a - b
        h *= 2
    return (v / divisor(n)).reshape(shape)


def hadamard_rows(x, n, sign=None):
    """the op: x fp16 or f32 [rows, cols] -> the same dtype"""
    assert x.dtype in (np.float16, np.float32) and x.ndim == 2
    with np.errstate(over="ignore"):
        return to_dtype(wht_f64(x, n, sign), x.dtype)


def hadamard_matrix(signs):
    """diag(s) H / d in f64: the reference's random_hadamard_matrix for these signs"""
    return wht_f64(np.diag(np.asarray(signs).astype(np.float64)), len(signs))


def layer_prefixes(sd):
    return [f"model.layers.{i}." for i in sorted({int(k.split(".")[2]) for k in sd if k.startswith("model.layers.")})]


def fuse_layer_norms(sd, tied=False):
    out = dict(sd)
    if tied or "lm_head.weight" not in sd:
        out["lm_head.weight"] = sd["model.embed_tokens.weight"].copy()

    def fuse(norm, linears):
        g = out[norm].astype(np.float64)
        for k in linears:
            out[k] = to_dtype(out[k].astype(np.float64) * g, out[k].dtype)
        out[norm] = np.ones_like(out[norm])

    for p in layer_prefixes(sd):
        for norm, linears in FUSED_BY.items():
            fuse(p + norm, [p + k for k in linears])
    fuse("model.norm.weight", ["lm_head.weight"])
    return out


def rotate_q(sd, hidden, signs):
    """the Q stage alone: W <- W Q on the input side, W <- Q^T W (and bias) on the output side of the residual stream"""
    out = dict(sd)
    for k, W in sd.items():
        tail = k.split(".", 3)[3] if k.startswith("model.layers.") and k.count(".") >= 4 else None
        if k in ("model.embed_tokens.weight", "lm_head.weight") or tail in RIGHT:
            out[k] = hadamard_rows(W, hidden, signs)
        elif tail in ("self_attn.o_proj.weight", "mlp.down_proj.weight"):
            out[k] = np.ascontiguousarray(hadamard_rows(np.ascontiguousarray(W.T), hidden, signs).T)
        elif tail in ("self_attn.o_proj.bias", "mlp.down_proj.bias"):
            out[k] = hadamard_rows(W[None, :], hidden, signs)[0]
    return out


def rotate_ov(sd, head_dim):
    """the per-head stage: v_proj on the output side (weight and bias), o_proj on the input side, blocks of head_dim"""
    out = dict(sd)
    for p in layer_prefixes(sd):
        v, o = p + "self_attn.v_proj.", p + "self_attn.o_proj."
        out[v + "weight"] = np.ascontiguousarray(hadamard_rows(np.ascontiguousarray(sd[v + "weight"].T), head_dim).T)
        if v + "bias" in sd:
            out[v + "bias"] = hadamard_rows(sd[v + "bias"][None, :], head_dim)[0]
        out[o + "weight"] = hadamard_rows(sd[o + "weight"], head_dim)
    return out


def rotate_model(sd, hidden, head_dim, signs, tied=False):
    return rotate_ov(rotate_q(fuse_layer_norms(sd, tied), hidden, signs), head_dim)
