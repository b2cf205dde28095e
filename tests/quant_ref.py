"""An exact restatement of the per-row int8 quantiser (include/qqq_amd.h, qqq_dynamic_quant) in numpy, the enumeration of the inputs at
which its kernels' shortcut needs its fallback, and fp16 rows built from them.

The contract:  s1 = f32(f16(f32(amax) * f32(1/127))),  q = clamp(round-half-even(x / s1), -128, 127),  a row whose scale is 0 -> codes 0.
quant_rows_exact() decides the rounding from exact integer-like products in float64; it shares no code with act_ref.quant_rows,
kv8_ref.quant_rows or the C oracle.

The kernels evaluate rint(f32(x) * f32(1 / s1)) and take the exact division only where |p - rint(p)| > 0.4995.  The product can land on
the wrong side of a half-integer only where x / s1 is exactly n + 1/2: an exact tie.  hard_ties() lists every exact tie of every reachable
scale and marks those at which the multiply-by-reciprocal rounds to the wrong integer (the hard ties): there a kernel whose fallback is
missing or mis-gated is wrong, and nowhere else.  corpus(L) packs them into rows of length L, edge_rows(L) adds the rows at the ends of
the format."""
import functools
from types import SimpleNamespace

import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64
R127 = F32(1) / F32(127)  # f32(1/127), what the kernels multiply amax by
GATE = F32(0.4995)
UNIT = 2.0 ** -24  # the smallest fp16 subnormal
_CHUNK = 1 << 17  # elements per pass of the row functions: the float64 temporaries stay in cache


def scale_of(amax):
    """f32 scale of fp16 amax (any shape)"""
    return (np.asarray(amax, F16).astype(F32) * R127).astype(F16).astype(F32)


def _row_chunks(y):
    y = np.asarray(y, F16)
    y2 = y.reshape(-1, y.shape[-1])
    step = max(1, _CHUNK // max(1, y2.shape[1]))
    return y, y2, [(i, min(i + step, y2.shape[0])) for i in range(0, y2.shape[0], step)]


def _exact(y2):
    """(round-half-even(x / s) as float64 with 0 where s == 0, f32 scales [m, 1], exact-tie mask) of fp16 rows [m, k]"""
    s32 = scale_of(np.abs(y2).max(axis=1, keepdims=True))
    live = s32 > 0
    s = np.where(live, s32, F32(1)).astype(F64)
    x = y2.astype(F64)
    n = np.floor(x / s)
    odd = (2.0 * n + 1.0) * s  # (2n + 1) s and 2x are exact in float64: 9 + 11 and 12 significant bits
    tie = (2.0 * x == odd) & live
    r = np.where(tie, n + np.mod(n, 2.0), n + (2.0 * x > odd))
    return np.where(live, r, 0.0), s32, tie


def quant_rows_hard(y):
    """(int8 codes y.shape, f32 scales y.shape[:-1] + (1,), hard-tie mask y.shape) of an fp16 array, every last-dim row on its own.  The
    mask is True where an element is an exact tie of its row's scale at which rint(f32(x) * f32(1 / s)) is the wrong integer."""
    y, y2, chunks = _row_chunks(y)
    codes = np.empty(y2.shape, np.int8)
    s1 = np.empty((y2.shape[0], 1), F32)
    hard = np.empty(y2.shape, bool)
    for a, b in chunks:
        r, s1[a:b], tie = _exact(y2[a:b])
        codes[a:b] = np.clip(r, -128, 127).astype(np.int8)
        rinv = F32(1) / np.where(s1[a:b] > 0, s1[a:b], F32(1))
        hard[a:b] = tie & (np.rint(y2[a:b].astype(F32) * rinv).astype(F64) != r)
    return codes.reshape(y.shape), s1.reshape(y.shape[:-1] + (1,)), hard.reshape(y.shape)


def quant_rows_exact(y):
    """(int8 codes y.shape, f32 scales y.shape[:-1] + (1,)) of an fp16 array, every last-dim row on its own"""
    return quant_rows_hard(y)[:2]


def shortcut_codes(y, gate=GATE):
    """The kernels' arithmetic in numpy: rint(f32(x) * f32(1 / s)), the exact f32 division where |p - rint(p)| > gate (gate=None: never)."""
    y, y2, chunks = _row_chunks(y)
    codes = np.empty(y2.shape, np.int8)
    for a, b in chunks:
        s32 = scale_of(np.abs(y2[a:b]).max(axis=1, keepdims=True))
        live = s32 > 0
        s = np.where(live, s32, F32(1))
        x = y2[a:b].astype(F32)
        p = x * (F32(1) / s)
        q = np.rint(p)
        if gate is not None:
            q = np.where(np.abs(p - q) > gate, np.rint(x / s), q)
        codes[a:b] = np.clip(np.where(live, q, F32(0)), -128, 127).astype(np.int8)
    return codes.reshape(y.shape)


def hard_tie_mask(y):
    """True where an element of an fp16 array is a hard tie of its row's scale"""
    return quant_rows_hard(y)[2]


def hard_tie_keys(y, mask=None):
    """the distinct (scale, x) pairs among the hard ties of an fp16 array, as sorted uint32 (f16 bits of the scale << 16 | f16 bits of x);
    mask: hard_tie_mask(y), where the caller has it"""
    y, y2, _ = _row_chunks(y)
    rows, cols = np.nonzero(hard_tie_mask(y2) if mask is None else np.asarray(mask).reshape(y2.shape))
    sb = scale_of(np.abs(y2).max(axis=1)).astype(F16).view(np.uint16).astype(np.uint32)
    return np.unique((sb[rows] << 16) | y2[rows, cols].view(np.uint16).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def hard_ties():
    """Every reachable non-zero scale with its smallest and largest amax, and every exact tie 0 < x <= that largest amax:
        scales f32 [S], amax_lo / amax_hi f16 [S], zero_amax (the largest amax whose scale is 0),
        scale_idx int [T], x f16 [T], n int [T] (x / s = n + 1/2), p f32 [T] (the shortcut's product),
        hard bool [T] (rint(p) is not round-half-even(n + 1/2)), flagged bool [T] (|p - rint(p)| > 0.4995)"""
    amax = np.arange(1, 0x7C00, dtype=np.uint16).view(F16)  # every positive finite fp16
    s_all = scale_of(amax)  # non-decreasing
    last = np.flatnonzero(np.r_[s_all[1:] != s_all[:-1], True])
    first = np.r_[0, last[:-1] + 1]
    live = s_all[last] > 0
    scales, amax_lo, amax_hi = s_all[last][live], amax[first][live], amax[last][live]
    n = np.arange(192, dtype=F64)  # amax / scale stays below 191
    c = (2.0 * n + 1.0)[None, :] * scales.astype(F64)[:, None] * 0.5  # (n + 1/2) s, exact
    with np.errstate(over="ignore"):
        xh = c.astype(F16)
    tie = (xh.astype(F64) == c) & (c <= amax_hi.astype(F64)[:, None])
    si, ni = np.nonzero(tie)
    x = xh[si, ni]
    p = x.astype(F32) * (F32(1) / scales[si])
    q = np.rint(p)
    want = (ni + ni % 2).astype(F32)
    return SimpleNamespace(scales=scales, amax_lo=amax_lo, amax_hi=amax_hi, zero_amax=amax[last][~live].max(), scale_idx=si, x=x, n=ni, p=p,
                           hard=q != want, flagged=np.abs(p - q) > GATE)


def brackets():
    """(scale f32 [B], x f16 [B]): for every reachable scale and every half-integer n + 1/2 below its largest amax / scale, the fp16 values
    next to (n + 1/2) s on both sides (the tie itself and its two neighbours where it is one).  x -> rint(f32(x / s)) and the exact
    rounding are both monotone, so if they agree on these they agree on every reachable (scale, x)."""
    t = hard_ties()
    n = np.arange(192, dtype=F64)
    c = (2.0 * n + 1.0)[None, :] * t.scales.astype(F64)[:, None] * 0.5
    hi = t.amax_hi.astype(F64)[:, None]
    ok = c <= hi
    si = np.nonzero(ok)[0]
    h = c[ok].astype(F16)
    with np.errstate(over="ignore"):
        near = np.stack([np.nextafter(h, F16(0)), h, np.nextafter(h, F16(np.inf))], 1)
    si = np.repeat(si, 3)
    near = near.reshape(-1)
    keep = (near > 0) & (near.astype(F64) <= t.amax_hi.astype(F64)[si])
    return t.scales[si[keep]], near[keep]


def _scale_values(t, i):
    """(ties of scale i in both signs with the hard ones first, the ties' fp16 neighbours in both signs) as fp16"""
    sel = t.scale_idx == i
    x, hard = t.x[sel], t.hard[sel]
    ties = np.concatenate([x[hard], x[~hard]])
    with np.errstate(over="ignore"):
        nb = np.unique(np.concatenate([np.nextafter(ties, F16(0)), np.nextafter(ties, F16(np.inf))]))
    nb = nb[(nb > 0) & (nb <= t.amax_hi[i]) & ~np.isin(nb, ties)]
    both = lambda v: np.stack([v, -v], 1).reshape(-1)
    return both(ties), both(nb)


@functools.lru_cache(maxsize=4)
def corpus(L):
    """fp16 rows [R, L] (L % 8 == 0, L >= 8), one or more per scale that has a hard tie, scale after scale.  A row of scale s holds + and -
    the largest amax of s at two places and L - 2 values of the sequence [hard ties of s, +-] [its other ties, +-] [the ties' fp16
    neighbours, +-] [+0, -0], cycled; a scale gets as many rows as its ties need, and the rows continue the sequence.  Row r is rotated by
    7 r elements, so that over the rows every element index holds the amax and the first (hard) ties.  corpus(L).scale_idx [R] is the
    index of each row's scale in hard_ties().scales.  The arrays are shared: do not write to them."""
    assert L % 8 == 0 and L >= 8, L
    t = hard_ties()
    rows, idx = [], []
    for i in np.unique(t.scale_idx[t.hard]):
        ties, nb = _scale_values(t, i)
        unit = np.concatenate([ties, nb, np.array([0.0, -0.0], F16)])
        nrows = -(-len(ties) // (L - 2))
        seq = np.resize(unit, nrows * (L - 2)).reshape(nrows, L - 2)  # np.resize repeats the unit
        for part in seq:
            row = np.empty(L, F16)
            row[0], row[L // 2] = t.amax_hi[i], -t.amax_hi[i]
            row[1:L // 2], row[L // 2 + 1:] = part[:L // 2 - 1], part[L // 2 - 1:]
            rows.append(np.roll(row, (7 * len(rows)) % L))
            idx.append(i)
    out = np.stack(rows)
    out.flags.writeable = False
    return SimpleNamespace(rows=out, scale_idx=np.array(idx))


def edge_rows(L):
    """fp16 rows [7, L] at the ends of the format: all +0; all -0; amax 63 * 2^-24 among other subnormals (scale 0); amax 64 * 2^-24 (the
    smallest non-zero scale); a row at s = 2^-24 with +-190, +-129, +-128 and +-127 units of 2^-24 (the clamp); amax 65504 in both signs;
    one non-zero element, in the last place"""
    assert L % 8 == 0 and L >= 8, L
    k = np.arange(L)
    sign = np.where(k % 3 == 0, -1.0, 1.0)
    rows = np.zeros((7, L), F64)
    rows[1] = -0.0
    rows[2] = sign * (1 + k % 62) * UNIT
    rows[2, L - 3], rows[2, 1] = 63 * UNIT, -63 * UNIT
    rows[3] = sign * (k % 64) * UNIT
    rows[3, L - 2] = 64 * UNIT
    rows[4] = sign * (k % 127) * UNIT
    rows[4, :8] = np.array([190, -190, 129, -129, 128, -128, 127, -127]) * UNIT
    rows[4] = np.roll(rows[4], L - 5)
    rows[5] = sign * (k % 97) * 512.0
    rows[5, 2], rows[5, L - 1] = 65504.0, -65504.0
    rows[6, L - 1] = -3.0
    out = rows.astype(F16)
    assert np.array_equal(out.astype(F64), rows)
    return out
