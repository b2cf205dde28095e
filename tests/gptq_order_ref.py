"""CPU restatement of GPTQ with act-order and static groups (qqq_amd/quant/include/qqq_amd_gptq_order.h and gptq_quantize_ordered) over
tests/gptq_ref.py, in the same numpy f32: the sweep with a scale per (row, column), every group's scale at once, and the reference's
fasterquant(actorder, static_groups) from the factor on.  The yardstick of tests/test_gptq_order_ref_cpu.py (against the fixture
recorded from the reference, tests/golden/gptq_order_small.npz) and of tests/test_gpu_gptq_order.py."""
import numpy as np

import gptq_ref as R

F32 = np.float32


def block_cols(W1, Hinv1, scale_cols):
    """gptq_ref.block in grouped arithmetic with the scale of step i taken from scale_cols[:, i] (f32 [rows, count]) -> (Q1, Err1)"""
    W1 = np.array(W1, F32)
    Hinv1 = np.asarray(Hinv1, F32)
    S = np.asarray(scale_cols, F32)
    assert S.shape == W1.shape
    Q1, Err1 = np.zeros_like(W1), np.zeros_like(W1)
    with np.errstate(all="ignore"):
        for i in range(W1.shape[1]):
            w = W1[:, i].copy()
            q = R.quantise(w, S[:, i], True)
            e = ((w - q) / Hinv1[i, i]).astype(F32)
            prod = (e[:, None] * Hinv1[i, i:][None, :]).astype(F32)  # rounded, THEN subtracted
            W1[:, i:] = W1[:, i:] - prod
            Q1[:, i], Err1[:, i] = q, e
    return Q1, Err1


def group_scales(W, mse=False):
    """f32 [rows, cols / 128]: the grouped scale of every 128-column group, each from its own 128 values"""
    W = np.asarray(W, F32)
    assert W.shape[1] % 128 == 0
    return np.stack([R.scales(W[:, g:g + 128], True, mse) for g in range(0, W.shape[1], 128)], axis=1).astype(F32)


def sweep_ordered(W, Hinv_perm, dead, perm=None, group_size=-1, mse=False, static_groups=True, gemm_dtype=np.float32, out_dtype=np.float16):
    """fasterquant(actorder = perm is not None, static_groups) from the factor on.  W f32-able [N, K] in natural order, `dead` the dead
    columns in natural order, `perm` the sweep order (None: no act-order), Hinv_perm the upper factor of the PERMUTED, damped Hessian.
    -> dict(weight [N, K] out_dtype, Q f32 -- both un-permuted --, Q_perm f32 in the swept order, scales f32 [N, G], s_extra or None).
    The order is the reference's: per-channel scales from the whole row, dead columns zeroed, static group scales from the unswept
    weight, the permutation, the sweep, the inverse permutation.  gemm_dtype as gptq_ref.sweep."""
    W = np.array(W, F32)
    N, K = W.shape
    grouped = group_size != -1
    if grouped and not static_groups:
        assert perm is None, "moving groups under act-order are not restated"
        r = R.sweep(W, Hinv_perm, dead, group_size, mse, gemm_dtype, out_dtype)
        return dict(r, Q_perm=r["Q"])
    sc = None if grouped else R.scales(W, False, mse)
    W[:, dead] = 0
    S = group_scales(W, mse) if grouped else None
    order = np.arange(K) if perm is None else np.asarray(perm, np.int64)
    W = W[:, order]
    Qp = np.zeros_like(W)
    for i1 in range(0, K, 128):
        i2 = min(i1 + 128, K)
        if grouped:
            Q1, Err1 = block_cols(W[:, i1:i2], Hinv_perm[i1:i2, i1:i2], S[:, order[i1:i2] // 128])
        else:
            Q1, Err1 = R.block(W[:, i1:i2], Hinv_perm[i1:i2, i1:i2], sc, False)
        Qp[:, i1:i2] = Q1
        if i2 < K:
            upd = Err1.astype(gemm_dtype) @ Hinv_perm[i1:i2, i2:].astype(gemm_dtype)
            W[:, i2:] = (W[:, i2:].astype(gemm_dtype) - upd).astype(F32) if gemm_dtype != np.float32 else W[:, i2:] - upd.astype(F32)
    Q = Qp[:, np.argsort(order)]
    weight = Q.astype(out_dtype)
    s = S if grouped else sc[:, None]
    s_extra = None
    if grouped:
        xmax = np.abs(weight.astype(F32)).max(axis=1, keepdims=True)
        s_extra = (np.where(xmax == 0, F32(1), xmax) / F32(127)).astype(F32)
    return dict(weight=weight, Q=Q, Q_perm=Qp, scales=s.astype(F32), s_extra=s_extra)


def hinv_of_permuted(H, perm=None, percdamp=0.01):
    """(Hinv f32 [K, K] upper of the permuted Hessian, dead columns in natural order, perm): the dead-column rule, the stable descending
    order of diag(H) where `perm` is None, then gptq_ref.hinv_of's damping and Cholesky chain on H[perm][:, perm]"""
    H = np.array(H, F32)
    dead = np.diag(H) == 0
    H[dead, dead] = 1
    if perm is None:
        perm = np.argsort(-np.diag(H), kind="stable")
    Hinv, _ = R.hinv_of(H[perm][:, perm], percdamp)
    return Hinv, dead, perm
