"""Beam search over the paged KV cache: QuantLlamaForCausalLM.beam_search (the reference's model.generate(num_beams=...), transformers'
rules).  The device does the step -- ops.beam_step behind every pass's logits -- and the block copies of PagedKVCache.reorder; the host
keeps the hypotheses.

    BeamHypothesis   (tokens, score, logprob) of one finished hypothesis
    blocks_needed    the blocks a prompt's beams can take at most: the admission rule
    beam_search      the call behind QuantLlamaForCausalLM.beam_search
"""
from __future__ import annotations

from collections import deque
from typing import List, NamedTuple, Optional, Sequence

import torch

from . import ops


class BeamHypothesis(NamedTuple):
    """A finished hypothesis: the generated tokens (the eos that ended it included), score = logprob / len(tokens) ** length_penalty, and
    logprob, the sum of the tokens' log-probabilities as the device added them up in f32."""
    tokens: List[int]
    score: float
    logprob: float


def blocks_needed(prompt_len: int, max_new_tokens: int, num_beams: int, block_size: int) -> int:
    """own + (num_beams - 1) * (own - prompt_len // block_size) with own = ceil((prompt_len + max_new_tokens - 1) / block_size): a beam
    holds at most prompt_len + max_new_tokens - 1 keys (the last token is never fed), and the prompt's full blocks are one copy for all
    beams, whatever the search does -- every beam descends from the prefilled one and reorder() shares full blocks by reference."""
    own = -(-(prompt_len + max_new_tokens - 1) // block_size)
    return own + (num_beams - 1) * (own - prompt_len // block_size)


class _Held:
    """the num_beams best finished hypotheses of one prompt (transformers' BeamHypotheses)"""

    def __init__(self, num_beams: int, length_penalty: float):
        self.num_beams, self.length_penalty, self.hyps = num_beams, length_penalty, []

    def add(self, tokens: List[int], logprob: float) -> None:
        score = logprob / len(tokens) ** self.length_penalty
        if len(self.hyps) < self.num_beams or score > self.worst():
            self.hyps.append(BeamHypothesis(tokens, score, logprob))
            if len(self.hyps) > self.num_beams:  # the worst goes, among equals the oldest
                del self.hyps[min(range(len(self.hyps)), key=lambda i: (self.hyps[i].score, i))]

    def full(self) -> bool:
        return len(self.hyps) >= self.num_beams

    def worst(self) -> float:
        return min(h.score for h in self.hyps)

    def best(self, n: int) -> List[BeamHypothesis]:
        return sorted(self.hyps, key=lambda h: -h.score)[:n]  # stable: among equals the oldest first


@torch.no_grad()
def beam_search(lm, prompts: Sequence[Sequence[int]], max_new_tokens: int, num_beams: int = 4, length_penalty: float = 1.0,
                early_stopping: bool = False, eos_token_id: Optional[int] = None, num_return_sequences: int = 1, cache=None,
                block_size: int = 16, dtype=torch.float16) -> List[List[BeamHypothesis]]:
    """QuantLlamaForCausalLM.beam_search: see there."""
    B, T, nret = int(num_beams), int(max_new_tokens), int(num_return_sequences)
    vocab = lm.lm_head.weight.shape[0]
    if B < 1 or B > 16 or 2 * B > vocab:
        raise ValueError(f"beam_search: num_beams={B} outside [1, min(16, vocab // 2 = {vocab // 2})]")
    if nret < 1 or nret > B:
        raise ValueError(f"beam_search: num_return_sequences={nret} outside [1, num_beams={B}]")
    eos = -1 if eos_token_id is None else int(eos_token_id)
    if eos_token_id is not None and not 0 <= eos < vocab:
        raise ValueError(f"beam_search: eos_token_id={eos} outside [0, vocab={vocab})")
    prompts = [list(p) for p in prompts]
    if any(not p for p in prompts):
        raise ValueError("beam_search: every prompt needs at least one token")
    results: List[List[BeamHypothesis]] = [[] for _ in prompts]
    if T < 1 or not prompts:
        return results
    lp_exp = float(length_penalty)
    dev = lm.lm_head.weight.device
    bs = cache.block_size if cache is not None else block_size
    bound = [blocks_needed(len(p), T, B, bs) for p in prompts]
    if cache is None:
        cache = lm.new_cache(sum(bound), block_size, dtype)
    tag = object()  # sequence ids no other user of the cache can hold
    sid = lambda p, b: (tag, p, b)  # noqa: E731
    held = [_Held(B, lp_exp) for _ in prompts]
    hist: List[List[List[int]]] = [[[]] * B for _ in prompts]  # per prompt and beam: the tokens so far
    count = [0] * len(prompts)                                 # ... and their number
    spaces = {}

    def step_on(logits, cum, live):
        rows = logits.shape[0]
        if rows not in spaces:
            spaces[rows] = ops.beam_step_workspace(rows, B, dev)
        return ops.beam_step(logits, cum, live, B, eos, spaces[rows])

    def release(p):
        for b in range(B):
            try:
                cache.free(sid(p, b))
            except KeyError:  # not forked yet, or never admitted
                pass

    def settle(group, step):
        """a pass's bookkeeping for the prompts of `group` (row g * B + b: beam b of group[g]) -> the positions in `group` that go on"""
        packed = step.packed.cpu()  # the pass's one read-back
        score, _, parent, token, next_parent = (x.tolist() for x in ops.unpack_beam_step(packed, len(group), B))
        keep, seqs, parents = [], [], []
        for g, p in enumerate(group):
            nxt = []
            for j in range(2 * B):
                if eos >= 0 and token[g][j] == eos:
                    if j < B:  # transformers' rule: an eos behind the first num_beams candidates is no hypothesis
                        held[p].add(hist[p][parent[g][j]] + [eos], score[g][j])
                    continue
                nxt.append(j)
                if len(nxt) == B:
                    break
            hist[p] = [hist[p][parent[g][j]] + [token[g][j]] for j in nxt]
            count[p] += 1
            done = held[p].full() and (early_stopping or not score[g][nxt[0]] / count[p] ** lp_exp > held[p].worst())
            if not done and count[p] >= T:  # the budget: the live beams finish as they are
                for b, j in enumerate(nxt):
                    held[p].add(hist[p][b], score[g][j])
                done = True
            if done:
                results[p] = held[p].best(nret)
                release(p)
                continue
            parents += [len(seqs) + b for b in next_parent[g * B:(g + 1) * B]]
            seqs += [sid(p, b) for b in range(B)]
            keep.append(g)
        if seqs:
            cache.reorder(seqs, parents)
        return keep

    def kept(step, keep, groups):
        ids, cum, live = step.next_ids, step.next_cum, step.next_live
        if len(keep) < groups:
            rows = torch.tensor([g * B + b for g in keep for b in range(B)], dtype=torch.int64).to(dev)
            ids, cum, live = ids[rows], cum[rows], live[rows]
        return ids, cum, live

    waiting, running = deque(range(len(prompts))), []
    cur = cum = live = None  # [len(running) * B] on the device: the beams' last tokens, summed log-probabilities and live flags
    try:
        while waiting or running:
            if running:
                seqs = [sid(p, b) for p in running for b in range(B)]
                step = step_on(lm(cur, cache, cache.step(seqs, [1] * len(seqs))), cum, live)
                keep = settle(running, step)
                cur, cum, live = kept(step, keep, len(running))
                running = [running[g] for g in keep]
            new = []
            owed = sum(bound[p] - len({blk for b in range(B) for blk in cache.blocks(sid(p, b))}) for p in running)
            while waiting and bound[waiting[0]] <= cache.free_blocks - owed:
                p = waiting.popleft()
                cache.add(sid(p, 0))
                owed += bound[p]
                new.append(p)
            if not new:
                if not running and waiting:
                    raise RuntimeError(f"beam_search: the pool's {cache.free_blocks} free blocks cannot hold a prompt that needs "
                                       f"{bound[waiting[0]]} (prompt, budget and beams)")
                continue
            ids = torch.tensor([t for p in new for t in prompts[p]], dtype=torch.int64, device=dev)
            logits = lm(ids, cache, cache.step([sid(p, 0) for p in new], [len(prompts[p]) for p in new]))
            rows = len(new) * B
            if B > 1:  # the prefill's row is beam 0's; the others are dead in this step and never read
                wide = logits.new_empty((rows, logits.shape[1]))
                wide[::B] = logits
                logits = wide
            first_live = torch.zeros(rows, dtype=torch.int32, device=dev)
            first_live[::B] = 1
            step = step_on(logits, torch.zeros(rows, dtype=torch.float32, device=dev), first_live)
            keep = settle(new, step)
            first = kept(step, keep, len(new))
            cur, cum, live = first if not running else (torch.cat(pair) for pair in zip((cur, cum, live), first))
            running = running + [new[g] for g in keep]
    except BaseException:  # leave the caller's pool as it was found
        for p in range(len(prompts)):
            release(p)
        raise
    return results


__all__ = ["BeamHypothesis", "beam_search", "blocks_needed"]
