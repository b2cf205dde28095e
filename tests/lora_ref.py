"""The f64 reference of ops.lora_add (include/qqq_amd_lora.h), the error bound an f32 implementation may use up, and the
cases tests/test_gpu_lora.py runs (tests/test_lora_ref_cpu.py holds the reference and the bound against them without a GPU).

    y[t, n] <- fp16( y[t, n] + scale[a] * sum_r B[a, n, r] * ( s1[t] * sum_k A[a, p * R + r, k] * xq[t, k] ) )      a = slot[t] >= 0

reference() computes the unrounded value in f64 from the same fp16 / int8 / f32 operands, and per element a bound on what f32 arithmetic
in ANY summation order may be off by, u = 2^-24:
    e_h[r]  = (K + 2) u s1 sum_k |A xq|                     the running-error bound of a K-term f32 sum, and the product with s1
    bound   = |scale| sum_r |B| e_h[r]                      that error carried through the outer sum
            + (R + 3) u |scale| sum_r |B| |h[r]|            the outer sum's own rounding, the product with scale
            + u (|y| + |scale sum_r B h|)                   the final add
check() passes a result that lies within half an fp16 ulp, at its own magnitude, of some value within `bound` of the reference.
The tolerance is derived from the operands, not measured on an implementation."""
import numpy as np

U = 2.0 ** -24
S = 17  # adapter slots of every case


def reference(y, xq, s1, A, B, scale, slot, part_cols):
    """-> (value f64 [T, N], bound f64 [T, N], touched bool [T]); rows with a slot outside [0, S) keep y exactly (bound 0)"""
    T, N = y.shape
    K = xq.shape[1]
    R = B.shape[2]
    val, bound = y.astype(np.float64), np.zeros((T, N))
    touched = np.zeros(T, dtype=bool)
    x = xq.astype(np.float64)
    for t in range(T):
        a = int(slot[t])
        if not 0 <= a < A.shape[0]:
            continue
        touched[t] = True
        s = float(s1.reshape(-1)[t])
        for p in range(len(part_cols) - 1):
            Ap = A[a, p * R:(p + 1) * R].astype(np.float64)
            h = s * (Ap @ x[t])
            e_h = (K + 2) * U * abs(s) * (np.abs(Ap) @ np.abs(x[t]))
            Bp = B[a, part_cols[p]:part_cols[p + 1]].astype(np.float64)
            acc = float(scale[a]) * (Bp @ h)
            y0 = val[t, part_cols[p]:part_cols[p + 1]].copy()
            val[t, part_cols[p]:part_cols[p + 1]] = y0 + acc
            bound[t, part_cols[p]:part_cols[p + 1]] = (abs(float(scale[a])) * (np.abs(Bp) @ e_h)
                                                        + (R + 3) * U * abs(float(scale[a])) * (np.abs(Bp) @ np.abs(h))
                                                        + U * (np.abs(y0) + np.abs(acc)))
    return val, bound, touched


def fp16_ulp(v):
    """the spacing of fp16 at the magnitude of v (f64 array): 2^(e - 10), 2^-24 in the subnormal range"""
    mag = np.maximum(np.abs(v), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(mag)) - 10)


def check(got, val, bound):
    """got fp16 [T, N] -> bool [T, N]: within half an fp16 ulp (at got's magnitude) of the interval [val - bound, val + bound]"""
    g = got.astype(np.float64)
    dist = np.maximum(np.abs(g - val) - bound, 0.0)
    return np.isfinite(g) & (dist <= 0.5 * fp16_ulp(g))


def slots_of(pattern, T):
    t = np.arange(T)
    if pattern == "none":
        s = np.full(T, -1)
    elif pattern == "same":
        s = np.full(T, 3)
    elif pattern == "distinct16":       # 16 different adapters in every 16-token tile
        s = (t * 5 + 1) % 16 + (t // 16) % 2
    elif pattern == "runs":             # runs of 6 tokens: they cross the 16-token tile boundaries
        s = (t // 6 * 7) % S
    elif pattern == "last":             # the last slot, and slot 0 on every fourth row
        s = np.where(t % 4 == 1, 0, S - 1)
    elif pattern == "interleaved":      # no adapter on every third row
        s = np.where(t % 3 == 0, -1, (t * 5) % S)
    else:
        raise ValueError(pattern)
    return s.astype(np.int32)


# (T, K, N, R, part_cols, slot pattern, row stride of y)
CASES = [
    (1, 128, 128, 8, (0, 128), "same", 128),
    (15, 192, 320, 16, (0, 320), "interleaved", 320),
    (16, 128, 128, 64, (0, 128), "distinct16", 128),
    (17, 192, 128, 16, (0, 128), "runs", 128),
    (70, 192, 320, 8, (0, 320), "runs", 330),
    (70, 128, 320, 64, (0, 320), "interleaved", 320),
    (2, 11008, 128, 16, (0, 128), "last", 128),
    (17, 128, 256, 16, (0, 128, 256), "runs", 256),
    (70, 192, 384, 8, (0, 256, 320, 384), "interleaved", 384),
    (16, 192, 384, 64, (0, 256, 320, 384), "distinct16", 390),
    (15, 128, 128, 16, (0, 128), "none", 128),
    (17, 128, 320, 16, (0, 320), "last", 320),
    (1, 192, 256, 64, (0, 128, 256), "same", 256),
]


def case_id(case):
    T, K, N, R, cols, pattern, ld = case
    return f"T{T}-K{K}-N{N}-R{R}-P{len(cols) - 1}-{pattern}" + (f"-ld{ld}" if ld != N else "")


def inputs(case, seed=0):
    """the operands of a case as numpy arrays: y fp16 [T, ld] (the op sees y[:, :N]), xq int8, s1 f32 [T, 1], A, B fp16, scale f32, slot int32"""
    T, K, N, R, cols, pattern, ld = case
    rng = np.random.default_rng([seed, T, K, N, R])
    P = len(cols) - 1
    y = (rng.standard_normal((T, ld)) * 2.0).astype(np.float16)
    y[0, 0] = np.float16(-0.0)
    xq = rng.integers(-127, 128, size=(T, K), dtype=np.int8)
    s1 = (rng.random((T, 1), dtype=np.float32) + 0.5) * np.float32(1.0 / (64.0 * np.sqrt(K)))
    A = (rng.standard_normal((S, P * R, K)) * 0.03).astype(np.float16)
    B = (rng.standard_normal((S, N, R)) * (0.5 / np.sqrt(R))).astype(np.float16)
    scale = (rng.random(S, dtype=np.float32) + 0.5) * np.float32(2.0)
    return dict(y=y, xq=xq, s1=s1, A=A, B=B, scale=scale, slot=slots_of(pattern, T), part_cols=cols, N=N)
