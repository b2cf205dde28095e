"""Scoring text with the whole model: per-token log-probabilities over the paged KV cache, and what evaluation builds from them -- the
log-likelihood of a continuation (lm-eval's request type) and the perplexity of the reference's examples/eval_model.py.

    pack_steps(lengths, chunk_tokens, block_size)   the plan: which tokens of which sequence go into which forward pass (pure host code)
    score(lm, sequences, ...)                       log p(seq[t + 1] | seq[:t + 1]) for every sequence, f32 [len - 1] each
    loglikelihood(lm, requests, ...)                (sum of the continuation's log-probs, is_greedy) per (context, continuation)
    perplexity(lm, token_ids, seqlen, ...)          exp(sum nll / (nsamples * seqlen)) over disjoint windows, the reference's convention

QuantLlamaForCausalLM.score / loglikelihood / perplexity delegate here.  Every forward pass of a plan is
cache.step -> lm(ids, cache, step, all_rows=True) -> ops.token_logprobs: the fp16 logits of a chunk are the only large temporary, there is
no fp32 copy of them, and per chunk only the targets' log-probabilities (and the argmax ids) stay.

The packing policy (fixed, so that a caller can rebuild the passes): sequences are taken in order; a step is filled up to `chunk_tokens`
tokens; a sequence that does not fit is split where the step fills and continues at the head of the next step.  So a step holds at most
one sequence that began earlier (its first entry) and at most one that goes on (its last entry), and every step but the last is full.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import ops
from .paged import PagedKVCache

Step = List[Tuple[int, int, int]]


def pack_steps(lengths: Sequence[int], chunk_tokens: int, block_size: int = 16) -> Tuple[List[Step], List[int]]:
    """The forward passes that score sequences of `lengths` tokens, at most `chunk_tokens` tokens per pass -> (steps, blocks).

    steps[s] is a list of (sequence index, start, count): the pass feeds tokens start ... start + count - 1 of that sequence, in this
    order (the module docstring states the policy).  blocks[s] is the number of cache blocks of `block_size` keys that are live during
    pass s: ceil((start + count) / block_size) for each of its entries -- a sequence takes its blocks as it grows and gives all of them back
    right after the pass that holds its last token.  max(blocks) is what a cache must have free.  Pure host code."""
    lengths = [int(n) for n in lengths]
    chunk_tokens, block_size = int(chunk_tokens), int(block_size)
    if chunk_tokens < 1:
        raise ValueError(f"pack_steps: chunk_tokens must be at least 1, not {chunk_tokens}")
    if block_size < 1:
        raise ValueError(f"pack_steps: block_size must be at least 1, not {block_size}")
    if any(n < 1 for n in lengths):
        raise ValueError("pack_steps: every sequence needs at least one token")
    steps: List[Step] = []
    cur: Step = []
    room = chunk_tokens
    for i, n in enumerate(lengths):
        start = 0
        while start < n:
            count = min(n - start, room)
            cur.append((i, start, count))
            start += count
            room -= count
            if room == 0:
                steps.append(cur)
                cur, room = [], chunk_tokens
    if cur:
        steps.append(cur)
    blocks = [sum(-(-(start + count) // block_size) for _, start, count in step) for step in steps]
    return steps, blocks


@torch.no_grad()
def score(lm, sequences: Sequence[Sequence[int]], cache: Optional[PagedKVCache] = None, chunk_tokens: int = 2048, block_size: int = 16,
          dtype=torch.float16, return_greedy: bool = False):
    """log p(seq[t + 1] | seq[:t + 1]) for t = 0 ... len - 2 of every sequence (token lists of any lengths >= 1) -> a list of f32 tensors
    [len - 1] on the model's device; with return_greedy=True (logprobs, greedy), greedy[i] the int64 [len - 1] argmax of the model at
    the same positions (the token generate() would emit there at temperature 0).

    The passes are pack_steps(lengths, chunk_tokens, block size of the cache).  A sequence is added to the cache when its first chunk is
    packed and freed right after the pass that holds its last chunk.  `cache`: a PagedKVCache to run in (it may hold other sequences; its
    block size and dtype apply); it must have max(blocks of the plan) free blocks, or this raises before anything is launched and leaves
    it unchanged; it comes back with the same free blocks.  Default: a new cache of exactly the plan's need (`block_size`, `dtype`).
    fuse_prefill() and the cache dtype are honoured as they are set: the numbers are those of the paths generation runs.
    Peak extra memory: the fp16 [chunk_tokens, vocab] logits of one pass and O(chunk_tokens) besides the results."""
    seqs = [list(s) for s in sequences]
    if any(not s for s in seqs):
        raise ValueError("score: every sequence needs at least one token")
    bs = cache.block_size if cache is not None else block_size
    steps, blocks = pack_steps([len(s) for s in seqs], chunk_tokens, bs)
    need = max(blocks, default=0)
    if cache is None:
        cache = lm.new_cache(max(need, 1), bs, dtype)
    elif need > cache.free_blocks:
        raise RuntimeError(f"score: the plan needs {need} free blocks of {bs} keys, the cache has {cache.free_blocks}")
    dev = lm.lm_head.weight.device
    tag = object()  # sequence ids no other user of the cache can hold
    sid = lambda i: (tag, i)  # noqa: E731
    lp_parts: List[List[torch.Tensor]] = [[] for _ in seqs]
    am_parts: List[List[torch.Tensor]] = [[] for _ in seqs]
    live = set()
    try:
        for step in steps:
            ids: List[int] = []
            targets: List[int] = []
            for i, start, count in step:
                if start == 0:
                    cache.add(sid(i))
                    live.add(i)
                s = seqs[i]
                ids += s[start:start + count]
                targets += s[start + 1:start + count + 1]
                if start + count == len(s):
                    targets.append(-1)  # nothing follows a sequence's last token: ignored by the kernel, dropped below
            pstep = cache.step([sid(i) for i, _, _ in step], [count for _, _, count in step])
            logits = lm(torch.tensor(ids, dtype=torch.int64, device=dev), cache, pstep, all_rows=True)
            lp, am = ops.token_logprobs(logits, torch.tensor(targets, dtype=torch.int64, device=dev), return_greedy)
            del logits
            row = 0
            for i, start, count in step:
                last = start + count == len(seqs[i])
                keep = count - 1 if last else count
                lp_parts[i].append(lp[row:row + keep])
                if return_greedy:
                    am_parts[i].append(am[row:row + keep])
                row += count
                if last:
                    cache.free(sid(i))
                    live.discard(i)
    finally:
        for i in live:  # a pass raised: the caller's cache gets its blocks back
            cache.free(sid(i))
    logprobs = [torch.cat(p) for p in lp_parts]
    if not return_greedy:
        return logprobs
    return logprobs, [torch.cat(p) for p in am_parts]


def loglikelihood(lm, requests: Sequence[Tuple[Sequence[int], Sequence[int]]], **score_kw) -> List[Tuple[float, bool]]:
    """lm-eval's loglikelihood request: for every (context_ids, continuation_ids), both non-empty ->
    (log p(continuation | context), the sum of the continuation tokens' log-probs, formed in f64; is_greedy: the continuation is what
    greedy decoding would have produced, token for token).  `score_kw` goes to score (cache, chunk_tokens, block_size, dtype)."""
    reqs = [(list(c), list(t)) for c, t in requests]
    if any(not c or not t for c, t in reqs):
        raise ValueError("loglikelihood: every request needs at least one context token and one continuation token")
    if not reqs:
        return []
    score_kw.pop("return_greedy", None)
    logprobs, greedy = score(lm, [c + t for c, t in reqs], return_greedy=True, **score_kw)
    out = []
    for (c, t), lp, am in zip(reqs, logprobs, greedy):
        k = len(c) - 1  # position k predicts the continuation's first token
        out.append((float(lp[k:].double().sum().item()), am[k:].tolist() == t))
    return out


def perplexity_from_logprobs(window_logprobs: Sequence, seqlen: int) -> float:
    """The reference's perplexity (examples/eval_model.py) from the log-probs of `nsamples` windows of `seqlen` tokens, seqlen - 1 targets
    each: per window nll = mean over its seqlen - 1 targets of -logprob, TIMES seqlen; ppl = exp(sum of nll / (nsamples * seqlen)).
    That is the exponential of the mean over windows of the per-target mean NLL -- every window weighs the same, and the factor seqlen
    cancels.  It is NOT exp of the mean over all targets of text scored with context carried across windows: each window starts
    without context.  Formed in f64."""
    nlls = []
    for lp in window_logprobs:
        lp = torch.as_tensor(lp).double().reshape(-1)
        if lp.numel() != seqlen - 1:
            raise ValueError(f"perplexity: a window of {seqlen} tokens has {seqlen - 1} targets, not {lp.numel()}")
        nlls.append(float((-lp).mean().item()) * seqlen)
    if not nlls:
        raise ValueError("perplexity: no window")
    return math.exp(sum(nlls) / (len(nlls) * seqlen))


def perplexity(lm, token_ids, seqlen: int = 2048, **score_kw) -> float:
    """The perplexity protocol of the reference's examples/eval_model.py, to the letter: token_ids (a tensor, array or list of any shape,
    read in order) is cut into numel // seqlen disjoint windows of seqlen tokens (a remainder is dropped), every window is scored
    without context from the one before, and the result is perplexity_from_logprobs -- the reference's convention, not the per-target
    mean over the text.  `score_kw` goes to score (cache, chunk_tokens, block_size, dtype)."""
    seqlen = int(seqlen)
    if seqlen < 2:
        raise ValueError(f"perplexity: seqlen must be at least 2, not {seqlen}")
    flat = torch.as_tensor(token_ids).reshape(-1).tolist()
    nsamples = len(flat) // seqlen
    if nsamples < 1:
        raise ValueError(f"perplexity: {len(flat)} tokens hold no window of {seqlen}")
    score_kw.pop("return_greedy", None)
    windows = [flat[i * seqlen:(i + 1) * seqlen] for i in range(nsamples)]
    return perplexity_from_logprobs([lp.cpu() for lp in score(lm, windows, **score_kw)], seqlen)


__all__ = ["pack_steps", "score", "loglikelihood", "perplexity", "perplexity_from_logprobs"]
