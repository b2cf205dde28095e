"""float64 numpy statement of one row of ops.sample_tokens (include/qqq_amd_sample.h): the surviving set, the running sum of the weights over
it in token-id order, and the token.  Written from the semantics, independently of the kernel: exact weights in float64, no fixed point, no
radix select."""
import numpy as np


def sample_row(logits, T, k, p, u):
    """logits: 1-d array (the fp16 values, any float dtype) -> dict(greedy, survive bool [vocab], c float64 [vocab] (running sum of the
    weights over the survivors in token-id order, 0-weight elsewhere), W2, token)."""
    l = np.asarray(logits, dtype=np.float64)
    vocab = l.shape[0]
    T, p, u = float(np.float32(T)), float(np.float32(p)), float(np.float32(u))
    l = np.where(np.isnan(l), -np.inf, l)  # NaN: no weight, smallest for top-k
    valid = l > -np.inf
    out = dict(greedy=False, survive=np.zeros(vocab, dtype=bool), c=np.zeros(vocab), W2=0.0, token=0)
    if not np.isfinite(l).any():
        return out
    lmax = l.max()
    if not (T > 0) or k == 1:
        out.update(greedy=True, token=int(np.argmax(l)))  # argmax: the first occurrence
        out["survive"][out["token"]] = True
        return out
    kept = valid.copy()
    if 0 < k < vocab:
        kth = np.sort(l)[vocab - k]
        kept &= l >= kth
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(l == lmax, 1.0, np.exp((l - lmax) / T))
    w = np.where(kept & ~np.isnan(w), w, 0.0)
    survive = kept.copy()
    if p < 1:  # false for NaN
        W = w.sum()
        order = np.argsort(l, kind="stable")
        csum = np.cumsum(w[order])
        # the mass of the kept tokens with l_i <= l_j: the cumulative sum at the LAST position of j's tie group
        ls = l[order]
        last = np.searchsorted(ls, l, side="right") - 1
        below = csum[last]
        survive &= below > (1.0 - p) * W
        survive |= kept & (l == lmax)
    ws = np.where(survive, w, 0.0)
    c = np.cumsum(ws)
    W2 = c[-1]
    uc = min(max(u, 0.0), float(np.nextafter(np.float32(1), np.float32(0)))) if u == u else 0.0
    hit = np.nonzero(survive & (c > uc * W2))[0]
    token = int(hit[0]) if hit.size else int(np.nonzero(survive)[0][-1])
    out.update(survive=survive, c=c, W2=W2, token=token)
    return out


def sample_rows(logits, T, k, p, u):
    """rows of logits [rows, vocab] with per-row or scalar parameters -> list of sample_row results"""
    logits = np.asarray(logits)
    rows = logits.shape[0]
    bc = lambda v: np.broadcast_to(np.asarray(v), (rows,))  # noqa: E731
    T, k, p, u = bc(T), bc(k), bc(p), bc(u)
    return [sample_row(logits[i], T[i], int(k[i]), p[i], u[i]) for i in range(rows)]
