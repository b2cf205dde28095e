"""Reference restatement in numpy of the q / k norm fused into the RoPE / cache-write ops (include_ops/qqq_amd_qknorm.h), written from the
header's text: the norm with its f64 sum in the stated lane order, then the rotation of include/qqq_amd_attn.h, then act_ref.quant_rows
for the int8 forms.  Rows are head rows: fp16 [rows, d], d in {64, 128}.

    sumsq(x)                 f64 [rows]: a lane's 8 low then 8 high squares onto 0.0, then the xor butterfly over lanes 1, 2, (P = 8) 4
    norm(x, w, eps)          fp16 [rows, d]: y = fp16(w * fp16(x * (1 / sqrt(float(ss / d) + eps))))
    rope(y, cos, sin)        fp16 [rows, d]: fp16(fp16(y * cos) + fp16(rotate_half(y) * sin)), cos / sin the rows' table rows
    rope_qkv_norm(...)       (q_rows [m, h, d], k_rows [m, kvh, d], v_rows [m, kvh, d]) of a call's m tokens: what q_out and the fp16
                             cache hold for each token, wherever the layout puts it
    quant(rows)              (int8 codes, f32 scales) of fp16 [..., d] rows: what the int8 cache holds for them
"""
import numpy as np

import act_ref

F16, F32, F64 = np.float16, np.float32, np.float64


def sumsq(x):
    x = np.asarray(x, F16)
    rows, d = x.shape
    assert d in (64, 128)
    P, hd = d // 16, d // 2
    x64 = x.astype(F64)
    sq = x64 * x64  # exact: an fp16 square has 22 significant bits
    lane = np.zeros((rows, P), F64)
    for i in range(P):
        for e in range(8):
            lane[:, i] = lane[:, i] + sq[:, 8 * i + e]
        for e in range(8):
            lane[:, i] = lane[:, i] + sq[:, hd + 8 * i + e]
    idx = np.arange(P)
    for step in (1, 2, 4):
        if step < P:
            lane = lane + lane[:, idx ^ step]
    assert (lane == lane[:, :1]).all()  # every lane of a head ends with the same bits
    return lane[:, 0]


def norm(x, w, eps):
    x = np.asarray(x, F16)
    d = x.shape[1]
    var = (sumsq(x) / F64(d)).astype(F32)[:, None]
    rs = F32(1) / np.sqrt(var + F32(eps), dtype=F32)
    n = (x.astype(F32) * rs).astype(F16)
    return (np.asarray(w, F16).astype(F32)[None, :] * n.astype(F32)).astype(F16)


def rope(y, cos, sin):
    y = np.asarray(y, F16)
    hd = y.shape[1] // 2
    rot = np.concatenate((-y[:, hd:], y[:, :hd]), axis=1)
    p0 = (y.astype(F32) * np.asarray(cos, F16).astype(F32)).astype(F16)
    p1 = (rot.astype(F32) * np.asarray(sin, F16).astype(F32)).astype(F16)
    return (p0.astype(F32) + p1.astype(F32)).astype(F16)


def rope_qkv_norm(q, k, v, q_weight, k_weight, eps, cos, sin, pos, h, kvh, d):
    """q [m, h*d], k, v [m, kvh*d] fp16, cos / sin [table_len, d], pos int [m], every position inside the table"""
    q, k, v = (np.asarray(t, F16) for t in (q, k, v))
    m = q.shape[0]
    pos = np.asarray(pos, np.int64)

    def one(x, heads, w):
        rows = x.reshape(m * heads, d)
        p = np.repeat(pos, heads)
        return rope(norm(rows, w, eps), np.asarray(cos)[p], np.asarray(sin)[p]).reshape(m, heads, d)

    return one(q, h, q_weight), one(k, kvh, k_weight), v.reshape(m, kvh, d).copy()


def quant(rows):
    rows = np.asarray(rows, F16)
    codes, scales = act_ref.quant_rows(rows.reshape(-1, rows.shape[-1]))
    return codes.reshape(rows.shape), scales.reshape(rows.shape[:-1])
