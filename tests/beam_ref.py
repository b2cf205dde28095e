"""Numpy reference of the beam-search step (include/qqq_amd_beam.h) and of a whole search, written from the definition.

    merge(ids, lps, cum, live, B, eos)      rules 2 - 5 on the rows' candidates: f32 arithmetic, exact.  With ids / lps from
                                            ops.topk_logprobs (rule 1: "that op's top_logprobs to the bit") it is what ops.beam_step must
                                            return bit for bit.
    beam_step(logits, cum, live, B, eos)    rule 1 from tests/logprobs_ref.py's topk_logprobs_row (float64 values, rounded to f32), then
                                            merge: exact in the ids wherever the f32 scores are apart, to score_ref.tolerance in the values.
    search(logits_fn, prompt, ...)          one prompt's whole search given logits_fn(tokens so far) -> a row of fp16 logits, with the
                                            hypothesis rules of QuantLlamaForCausalLM.beam_search.
"""
import numpy as np

import logprobs_ref


def order_value(score) -> float:
    """what rule 3 compares: NaN and -inf are -inf (equal, below everything), -0 is +0"""
    s = float(score)
    return float("-inf") if np.isnan(s) else s + 0.0


def merge(ids, lps, cum, live, B: int, eos: int = -1):
    """ids int [P * B, 2B], lps f32 [P * B, 2B] (a dead row's are ignored), cum f32 [P * B], live int [P * B] -> dict of the op's outputs."""
    ids, lps = np.asarray(ids), np.asarray(lps, np.float32)
    cum, live = np.asarray(cum, np.float32), np.asarray(live)
    rows, k = lps.shape
    assert k == 2 * B and rows % B == 0
    P = rows // B
    out = dict(cand_score=np.full((P, k), -np.inf, np.float32), cand_logprob=np.full((P, k), -np.inf, np.float32),
               cand_parent=np.full((P, k), -1, np.int32), cand_token=np.full((P, k), -1, np.int32),
               next_ids=np.zeros(rows, np.int64), next_parent=np.full(rows, -1, np.int32), next_cum=np.full(rows, -np.inf, np.float32),
               next_live=np.zeros(rows, np.int32))
    for p in range(P):
        cands = []
        for b in range(B):
            r = p * B + b
            if not live[r]:
                continue
            for i in range(k):
                with np.errstate(invalid="ignore", over="ignore"):
                    score = np.float32(cum[r] + lps[r, i])  # one f32 addition
                cands.append((-order_value(score), b, i, score))
        if not cands:
            continue
        cands.sort(key=lambda c: c[:3])
        assert len(cands) >= k
        place = 0
        for j, (_, b, i, score) in enumerate(cands[:k]):
            r = p * B + b
            out["cand_score"][p, j], out["cand_logprob"][p, j] = score, lps[r, i]
            out["cand_parent"][p, j], out["cand_token"][p, j] = b, ids[r, i]
            if not (eos >= 0 and ids[r, i] == eos) and place < B:
                o = p * B + place
                out["next_ids"][o], out["next_parent"][o], out["next_cum"][o], out["next_live"][o] = ids[r, i], b, score, 1
                place += 1
        assert place == B  # a live beam contributes eos at most once
    return out


def row_candidates(logits: np.ndarray, live, B: int):
    """rule 1 from the float64 reference: (ids int64 [rows, 2B], lps f32 [rows, 2B]); a dead row's are zeros"""
    rows = logits.shape[0]
    ids, lps = np.zeros((rows, 2 * B), np.int64), np.zeros((rows, 2 * B), np.float32)
    for r in range(rows):
        if live[r]:
            _, _, ids[r], vals = logprobs_ref.topk_logprobs_row(logits[r], None, 2 * B)
            lps[r] = vals.astype(np.float32)
    return ids, lps


def beam_step(logits: np.ndarray, cum, live, B: int, eos: int = -1):
    ids, lps = row_candidates(logits, live, B)
    return merge(ids, lps, cum, live, B, eos)


class Held:
    """the B best finished hypotheses (tokens, score, logprob) of a prompt"""

    def __init__(self, B, length_penalty):
        self.B, self.lp, self.hyps = B, length_penalty, []

    def add(self, tokens, logprob):
        score = logprob / len(tokens) ** self.lp
        if len(self.hyps) < self.B or score > min(h[1] for h in self.hyps):
            self.hyps.append((list(tokens), score, logprob))
            if len(self.hyps) > self.B:
                worst = min(h[1] for h in self.hyps)
                del self.hyps[[h[1] for h in self.hyps].index(worst)]  # among equals the oldest

    def best(self, n):
        return sorted(self.hyps, key=lambda h: -h[1])[:n]


def search(logits_fn, prompt, max_new_tokens: int, B: int, length_penalty: float = 1.0, early_stopping: bool = False, eos: int = -1,
           num_return: int = 1, step=None):
    """One prompt's search -> [(tokens, score, logprob)] best first.  `step(logits [B, vocab], cum, live)` -> merge()'s dict; default:
    beam_step above."""
    step = step or (lambda logits, cum, live: beam_step(logits, cum, live, B, eos))
    held = Held(B, length_penalty)
    beams = [list(prompt)] + [None] * (B - 1)  # the first pass: beam 0 alone is live
    cum, live = np.zeros(B, np.float32), np.array([1] + [0] * (B - 1), np.int32)
    n = len(prompt)
    for count in range(1, max_new_tokens + 1):
        rows = [logits_fn(b) if l else None for b, l in zip(beams, live)]
        width = next(r for r in rows if r is not None).shape[0]
        logits = np.stack([r if r is not None else np.zeros(width, np.float16) for r in rows])
        out = step(logits, cum, live)
        taken = 0
        for j in range(2 * B):
            if eos >= 0 and out["cand_token"][0, j] == eos:
                if j < B:
                    held.add(beams[out["cand_parent"][0, j]][n:] + [eos], float(out["cand_score"][0, j]))
                continue
            taken += 1
            if taken == B:
                break
        beams = [beams[out["next_parent"][b]] + [int(out["next_ids"][b])] for b in range(B)]
        cum, live = out["next_cum"], out["next_live"]
        if len(held.hyps) >= B and (early_stopping or not float(cum[0]) / count ** length_penalty > min(h[1] for h in held.hyps)):
            break
        if count == max_new_tokens:
            for b in range(B):
                held.add(beams[b][n:], float(cum[b]))
    return held.best(num_return)
