"""CPU restatement of the rotation op for blocks of n = K * 2^p columns and of the Q stage that uses it, in numpy f64
(qqq_amd/quant/include_ext/qqq_amd_rotate_k.h, qqq_amd/quant/rotation.py mode="hadamard_k"): the Sylvester stages of every sub-block in the
stated order, the table's signed adds with k' ascending, one divide, the two-step rounding.  The tests hold the HIP op to it bit for bit,
and hold it to the fixture recorded from the reference's own rotation (tests/golden/rotate_k_small.npz, gen_rotate_k_golden.py)."""
import numpy as np

import rotate_ref as R


def mix_f64(v, table, m, sign=None):
    """every block of n = K m consecutive entries of the last axis of v, in f64: (v * sign), the stages h = 1 ... m/2 inside every
    sub-block of m entries, then z[k m + c] = s(k,0) t[c] + s(k,1) t[m + c] + ... (one add per term, k' ascending), then / d"""
    table = np.asarray(table)
    K = table.shape[0]
    assert table.shape == (K, K) and m >= 1 and m & (m - 1) == 0
    n = K * m
    v = np.array(v, dtype=np.float64)
    shape = v.shape
    assert shape[-1] % n == 0
    v = v.reshape(-1, n)
    if sign is not None:
        v = v * np.asarray(sign).astype(np.float64)
    h = 1
    while h < m:
        w = v.reshape(-1, n // (2 * h), 2, h)
        a, b = w[:, :, 0, :].copy(), w[:, :, 1, :].copy()
        w[:, :, 0, :] = a + b  # i with (i & h) == 0
        w[:, :, 1, :] = a - b
        h *= 2
    t = v.reshape(-1, K, m)
    z = np.empty_like(t)
    for k in range(K):
        acc = np.where(table[k, 0] < 0, -t[:, 0, :], t[:, 0, :])  # a sign flip: zeros keep theirs
        for kk in range(1, K):
            acc = acc + np.where(table[k, kk] < 0, -t[:, kk, :], t[:, kk, :])
        z[:, k, :] = acc
    return (z.reshape(-1, n) / R.divisor(n)).reshape(shape)


def hadamard_rows_k(x, m, table, sign=None):
    """the op: x fp16 or f32 [rows, cols] -> the same dtype"""
    assert x.dtype in (np.float16, np.float32) and x.ndim == 2
    with np.errstate(over="ignore", invalid="ignore"):
        return R.to_dtype(mix_f64(x, table, m, sign), x.dtype)


def hadamard_matrix_k(signs, table, m):
    """diag(s) (table^T (x) H_m) / d in f64: the reference's random_hadamard_matrix for these signs when table is its hadK"""
    return mix_f64(np.diag(np.asarray(signs).astype(np.float64)), table, m)


def recover_table(Q, signs, K):
    """the K x K table behind a recorded Q = diag(s) (table^T (x) H_m) / d: table[k][k'] = s[k' m] * sign(Q[k' m, k m])"""
    m = Q.shape[0] // K
    s = np.asarray(signs).astype(np.int64)
    return np.array([[s[kk * m] * (1 if Q[kk * m, k * m] > 0 else -1) for kk in range(K)] for k in range(K)], dtype=np.int8)


def rotate_q(sd, hidden, signs, table):
    """the Q stage alone with a table: W <- W Q on the input side, W <- Q^T W (and bias) on the output side of the residual stream"""
    m = hidden // np.asarray(table).shape[0]
    op = lambda W: hadamard_rows_k(W, m, table, signs)
    out = dict(sd)
    for k, W in sd.items():
        tail = k.split(".", 3)[3] if k.startswith("model.layers.") and k.count(".") >= 4 else None
        if k in ("model.embed_tokens.weight", "lm_head.weight") or tail in R.RIGHT:
            out[k] = op(W)
        elif tail in ("self_attn.o_proj.weight", "mlp.down_proj.weight"):
            out[k] = np.ascontiguousarray(op(np.ascontiguousarray(W.T)).T)
        elif tail in ("self_attn.o_proj.bias", "mlp.down_proj.bias"):
            out[k] = op(W[None, :])[0]
    return out


def rotate_model(sd, hidden, head_dim, signs, table, tied=False):
    return R.rotate_ov(rotate_q(R.fuse_layer_norms(sd, tied), hidden, signs, table), head_dim)
