"""Float64 numpy reference of the scoring kernel's per-row semantics (include/qqq_amd_score.h), written from the definition: plain
exponentials and a plain logarithm, no fixed point, no truncation."""
import numpy as np


def token_logprob_row(l: np.ndarray, t: int):
    """One row of fp16 logits [vocab] and a target -> (logprob as float64, argmax)."""
    x = np.asarray(l).astype(np.float64)
    vocab = x.shape[0]
    valid = ~np.isnan(x) & (x > -np.inf)  # NaN and -inf have no weight
    argmax = int(np.where(valid, x, -np.inf).argmax()) if valid.any() else 0  # the lowest index of the maximum; -0 == +0
    t = int(t)
    if t < 0:
        return 0.0, argmax  # ignored, as with ignore_index
    if t >= vocab or not valid.any():
        return float("nan"), argmax
    if not valid[t]:
        return float("-inf"), argmax
    lmax = x[valid].max()
    if np.isposinf(lmax):  # the tie group of +inf shares the mass; finite logits have none
        return (-np.log(float(np.isposinf(x).sum())) if np.isposinf(x[t]) else float("-inf")), argmax
    W = np.exp(x[valid] - lmax).sum()
    return float((x[t] - lmax) - np.log(W)), argmax


def token_logprobs(logits: np.ndarray, targets):
    """Rows of fp16 logits [rows, vocab] and targets [rows] -> (logprob float64 [rows], argmax int64 [rows])."""
    out = [token_logprob_row(row, t) for row, t in zip(logits, targets)]
    return np.array([o[0] for o in out], np.float64), np.array([o[1] for o in out], np.int64)


def tolerance(ref):
    """The bound on |kernel - reference| (derived in tests/test_gpu_score.py): 8e-6 + 2^-23 |ref|."""
    return 8e-6 + 2.0 ** -23 * np.abs(ref)
