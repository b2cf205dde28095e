"""CPU restatement of the GPTQ quantiser's arithmetic (qqq_amd/quant/include/qqq_amd_quant.h), in numpy f32 -- one IEEE operation per
numpy call, so nothing is contracted -- with torch-CPU only where the library matters (pow and the f32 row sums of the shrink search, the
Cholesky steps).  The yardstick of tests/test_gptq_ref_cpu.py (against the fixture recorded from the reference) and of the GPU tests."""
import numpy as np
import torch

F32 = np.float32
GRID = 80


def quantise(w, s, grouped):
    """s * clamp(rint(w / s), -7, 7)  |  s * (clamp(rint(w / s) + 8, 0, 15) - 8), every step rounded to f32"""
    w, s = np.asarray(w, F32), np.asarray(s, F32)
    with np.errstate(all="ignore"):
        r = np.rint(w / s)
        if grouped:
            return (s * (np.clip(r + F32(8), F32(0), F32(15)) - F32(8))).astype(F32)
        return (s * np.clip(r, F32(-7), F32(7))).astype(F32)


def scale_of(rng, grouped):
    rng = np.asarray(rng, F32)
    return ((rng + rng) / F32(15)).astype(F32) if grouped else (rng / F32(7)).astype(F32)


def row_xmax(W):
    xmax = np.abs(np.asarray(W, F32)).max(axis=1)
    return np.where(xmax == 0, F32(1), xmax).astype(F32)


def candidates(W, grouped):
    """f32 [rows, 80]: the scale of every candidate of the shrink search"""
    xmax = row_xmax(W)
    p = np.array([F32(1 - i / 100) for i in range(GRID)], F32)
    return scale_of(p[None, :] * xmax[:, None], grouped)


def errors_f64(W, grouped):
    """f64 [rows, 80]: sum |q - w| ^ 2.4 of every candidate with the sum and the power in f64 (q itself is the f32 quantiser's)"""
    W = np.asarray(W, F32)
    cand = candidates(W, grouped)
    out = np.empty(cand.shape, np.float64)
    for i in range(GRID):
        q = quantise(W, cand[:, i:i + 1], grouped)
        out[:, i] = (np.abs(q.astype(np.float64) - W.astype(np.float64)) ** 2.4).sum(axis=1)
    return out


def scales(W, grouped, mse=False, return_index=False):
    """f32 [rows]: the scale of every row; with mse the reference's search -- f32 errors, strict <, so the earliest least"""
    W = np.asarray(W, F32)
    cand = candidates(W, grouped)
    if not mse:
        return (cand[:, 0], np.zeros(W.shape[0], np.int64)) if return_index else cand[:, 0]
    best = np.full(W.shape[0], np.inf, F32)
    idx = np.zeros(W.shape[0], np.int64)
    Wt = torch.from_numpy(W)
    for i in range(GRID):
        q = torch.from_numpy(quantise(W, cand[:, i:i + 1], grouped))
        err = (q - Wt).abs_().pow_(2.4).sum(1).numpy()
        better = err < best
        best[better], idx[better] = err[better], i
    s = cand[np.arange(W.shape[0]), idx]
    return (s, idx) if return_index else s


def block(W1, Hinv1, scale, grouped):
    """the column sweep of one block -> (Q1, Err1), f32 [rows, count]"""
    W1 = np.array(W1, F32)
    Hinv1 = np.asarray(Hinv1, F32)
    s = np.asarray(scale, F32).reshape(-1)
    Q1, Err1 = np.zeros_like(W1), np.zeros_like(W1)
    with np.errstate(all="ignore"):
        for i in range(W1.shape[1]):
            w = W1[:, i].copy()
            q = quantise(w, s, grouped)
            e = ((w - q) / Hinv1[i, i]).astype(F32)
            prod = (e[:, None] * Hinv1[i, i:][None, :]).astype(F32)  # rounded, THEN subtracted
            W1[:, i:] = W1[:, i:] - prod
            Q1[:, i], Err1[:, i] = q, e
    return Q1, Err1


def hinv_of(H, percdamp=0.01):
    """(Hinv f32 [K, K] upper, dead columns): the reference's dead-column rule, damping and three Cholesky steps on the CPU"""
    H = torch.from_numpy(np.array(H, F32))
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    damp = percdamp * torch.mean(torch.diag(H))
    d = torch.arange(H.shape[0])
    H[d, d] += damp
    H = torch.linalg.cholesky(H)
    H = torch.cholesky_inverse(H)
    return np.ascontiguousarray(torch.linalg.cholesky(H, upper=True).numpy()), dead.numpy()


def sweep(W, Hinv, dead, group_size=-1, mse=False, gemm_dtype=np.float32, out_dtype=np.float16):
    """fasterquant from the factor on: W f32-able [N, K] -> dict(weight [N, K] out_dtype, Q f32, scales f32 [N, G], s_extra or None).
    gemm_dtype: the precision of the trailing Err1 @ Hinv between blocks (f32 as the reference; f64 measures what its rounding moves)."""
    W = np.array(W, F32)
    N, K = W.shape
    grouped = group_size != -1
    sc = None if grouped else scales(W, False, mse)
    W[:, dead] = 0
    Q = np.zeros_like(W)
    group_scales = []
    for i1 in range(0, K, 128):
        i2 = min(i1 + 128, K)
        if grouped:
            sc = scales(W[:, i1:i2], True, mse)
            group_scales.append(sc)
        Q1, Err1 = block(W[:, i1:i2], Hinv[i1:i2, i1:i2], sc, grouped)
        Q[:, i1:i2] = Q1
        if i2 < K:
            upd = Err1.astype(gemm_dtype) @ Hinv[i1:i2, i2:].astype(gemm_dtype)
            W[:, i2:] = (W[:, i2:].astype(gemm_dtype) - upd).astype(F32) if gemm_dtype != np.float32 else W[:, i2:] - upd.astype(F32)
    weight = Q.astype(out_dtype)
    s = np.stack(group_scales, axis=1) if grouped else sc[:, None]
    s_extra = None
    if grouped:
        xmax = np.abs(weight.astype(F32)).max(axis=1, keepdims=True)
        s_extra = (np.where(xmax == 0, F32(1), xmax) / F32(127)).astype(F32)
    return dict(weight=weight, Q=Q, scales=s.astype(F32), s_extra=s_extra)


def codes(weight, s, grouped):
    """int8 [N, K]: the codes a fake-quantised weight stands for under scales [N, G] (what QuantLinear.pack stores)"""
    w = np.asarray(weight).astype(F32)
    s = np.repeat(np.asarray(s, F32), 128, axis=1) if grouped else np.asarray(s, F32)
    r = np.rint(w / s)
    return (np.clip(r + 8, 0, 15) if grouped else np.clip(r, -7, 7)).astype(np.int8)


def proxy_loss(W, Wq, H):
    """tr((W - Q) H (W - Q)^T) in f64"""
    D = np.asarray(W, np.float64) - np.asarray(Wq, np.float64)
    return float(np.einsum("ik,kl,il->", D, np.asarray(H, np.float64), D))
