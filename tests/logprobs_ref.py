"""Float64 numpy reference of the top-k log-probability kernel's per-row semantics (include/qqq_amd_logprobs.h), written from the
definition: the values are tests/score_ref.py's, the order is a sort on (-value, index) with -0 equal to +0 and NaN and -inf last."""
import numpy as np

import score_ref


def order_values(l: np.ndarray) -> np.ndarray:
    """One row of fp16 logits -> what the order compares, as float64: NaN and -inf become -inf (equal among themselves), -0 becomes +0."""
    x = np.asarray(l).astype(np.float64)
    return np.where(np.isnan(x), -np.inf, x) + 0.0


def order(l: np.ndarray) -> np.ndarray:
    """Every token of the row, by logit descending and then index ascending."""
    v = order_values(l)
    return np.lexsort((np.arange(v.shape[0]), -v))


def rank_row(l: np.ndarray, t: int) -> int:
    v = order_values(l)
    t = int(t)
    return 1 + int((v > v[t]).sum()) if 0 <= t < v.shape[0] else 0


def topk_logprobs_row(l: np.ndarray, t, k: int):
    """One row, a token (or None) and k -> (logprob float64 or None, rank or None, top_ids int64 [k], top_logprobs float64 [k])."""
    ids = order(l)[:k]
    vals = np.array([score_ref.token_logprob_row(l, int(j))[0] for j in ids], np.float64)
    if t is None:
        return None, None, ids.astype(np.int64), vals
    return score_ref.token_logprob_row(l, int(t))[0], rank_row(l, t), ids.astype(np.int64), vals


def topk_logprobs(logits: np.ndarray, tokens, k: int):
    """Rows of fp16 logits [rows, vocab], tokens [rows] or None, k -> (logprob float64 [rows], rank int64 [rows], top_ids int64 [rows, k],
    top_logprobs float64 [rows, k]); the first two None without tokens."""
    out = [topk_logprobs_row(row, None if tokens is None else tokens[r], k) for r, row in enumerate(logits)]
    ids = np.array([o[2] for o in out], np.int64).reshape(len(out), k)
    vals = np.array([o[3] for o in out], np.float64).reshape(len(out), k)
    if tokens is None:
        return None, None, ids, vals
    return np.array([o[0] for o in out], np.float64), np.array([o[1] for o in out], np.int64), ids, vals
