"""QuantLlamaForCausalLM.beam_search on the GPU, on the two-layer model of tests/test_gpu_model.py: token for token, and bit for bit in
logprob, against a reference search written here.  The reference drives the same model's forward over the same rows in the same order,
takes every row's candidates from ops.topk_logprobs (rule 1 of include/qqq_amd_beam.h), selects on the CPU with
tests/beam_ref.py's merge and keeps the hypotheses with its Held, and manages the cache with fork / free alone."""
import numpy as np
import pytest
import torch

import beam_ref
from test_gpu_model import VOCAB, _make_lm

pytestmark = pytest.mark.gpu

PROMPT_LENS = (5, 14, 33)  # 14: the beams cross a block boundary in the third pass; 33: a partial block from the start


def _prompts(seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in PROMPT_LENS]


def _reference(lm, prompts, T, B, eos, lp, early, nret, dtype):
    from qqq_amd import ops

    dev = lm.lm_head.weight.device
    cache = lm.new_cache(400, 16, dtype)
    P = len(prompts)
    held = [beam_ref.Held(B, lp) for _ in prompts]
    results = [None] * P
    gen = 0
    names = {(p, 0): ("r", p, 0, gen) for p in range(P)}  # (prompt, beam) -> the sequence that holds it now
    for sid in names.values():
        cache.add(sid)
    running = list(range(P))
    logits = lm(torch.tensor([t for q in prompts for t in q], dtype=torch.int64, device=dev), cache,
                cache.step([names[p, 0] for p in running], [len(q) for q in prompts]))
    hist = {p: [[]] * B for p in running}
    cum = {p: np.zeros(B, np.float32) for p in running}
    live = {p: np.array([1] + [0] * (B - 1), np.int32) for p in running}
    for count in range(1, T + 1):
        _, _, ids, lps = ops.topk_logprobs(logits, None, 2 * B)
        ids, lps = ids.cpu().numpy(), lps.cpu().numpy()
        if count == 1:  # one row per prompt: beam 0's
            wide_ids, wide_lps = np.zeros((len(running) * B, 2 * B), ids.dtype), np.zeros((len(running) * B, 2 * B), lps.dtype)
            wide_ids[::B], wide_lps[::B] = ids, lps
            ids, lps = wide_ids, wide_lps
        out = beam_ref.merge(ids, lps, np.concatenate([cum[p] for p in running]), np.concatenate([live[p] for p in running]), B, eos)
        gen += 1
        goes_on, feed = [], []
        for g, p in enumerate(running):
            taken = 0
            for j in range(2 * B):
                if eos >= 0 and out["cand_token"][g, j] == eos:
                    if j < B:
                        held[p].add(hist[p][out["cand_parent"][g, j]] + [eos], float(out["cand_score"][g, j]))
                    continue
                taken += 1
                if taken == B:
                    break
            rows = slice(g * B, (g + 1) * B)
            parents, toks = out["next_parent"][rows].tolist(), out["next_ids"][rows].tolist()
            hist[p] = [hist[p][b] + [t] for b, t in zip(parents, toks)]
            cum[p], live[p] = out["next_cum"][rows], out["next_live"][rows]
            done = len(held[p].hyps) >= B and (early or not float(cum[p][0]) / count ** lp > min(h[1] for h in held[p].hyps))
            if not done and count == T:
                for b in range(B):
                    held[p].add(hist[p][b], float(cum[p][b]))
                done = True
            old = {b: names.pop((p, b)) for b in range(B) if (p, b) in names}
            if not done:  # fork every next beam from its parent, then free the parents
                for b, parent in enumerate(parents):
                    names[p, b] = ("r", p, b, gen)
                    cache.fork(old[parent], names[p, b])
                goes_on.append(p)
                feed += toks
            else:
                results[p] = held[p].best(nret)
            for sid in old.values():
                cache.free(sid)
        running = goes_on
        if not running:
            break
        seqs = [names[p, b] for p in running for b in range(B)]
        logits = lm(torch.tensor(feed, dtype=torch.int64, device=dev), cache, cache.step(seqs, [1] * len(seqs)))
    assert cache.free_blocks == 400
    return results


@pytest.fixture(scope="module")
def lms(dev):
    return {gs: _make_lm(dev, gs) for gs in (-1, 128)}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
@pytest.mark.parametrize("gs", [-1, 128])
def test_beam_search_equals_the_reference_search(dev, lms, gs, dtype, fused):
    lm = lms[gs]
    for layer in lm.model.layers:
        (layer.fuse_prefill if fused else layer.unfuse_prefill)()
        (layer.fuse_decode if fused else layer.unfuse_decode)()
    prompts, T, B = _prompts(), 7, 4
    with torch.no_grad():
        free_run = lm.generate(prompts, T, dtype=dtype)
        eos = free_run[1][3]  # a token the greedy path of prompt 1 emits: hypotheses finish early somewhere
        cache = lm.new_cache(120, 16, dtype)
        cache.add("foreign")
        cache.step(["foreign"], [21])
        for pools in cache._pools():
            for pool in pools:
                pool[cache.blocks("foreign")] = 3
        foreign = [pool[cache.blocks("foreign")].clone() for pools in cache._pools() for pool in pools]
        free = cache.free_blocks
        for lp, early, nret in ((1.0, False, 4), (0.0, True, 2)):
            got = lm.beam_search(prompts, T, num_beams=B, length_penalty=lp, early_stopping=early, eos_token_id=eos, num_return_sequences=nret,
                                 cache=cache)
            want = _reference(lm, prompts, T, B, eos, lp, early, nret, dtype)
            assert [[(h.tokens, h.score) for h in r] for r in got] == [[(h[0], h[1]) for h in r] for r in want]
            for r, w in zip(got, want):  # logprob bit for bit: both are the f32 sums of the same f32 values
                assert np.array_equal(np.array([h.logprob for h in r], np.float32).view(np.uint32),
                                      np.array([h[2] for h in w], np.float32).view(np.uint32))
            assert cache.free_blocks == free and cache.length("foreign") == 21  # all blocks are back, the foreign sequence is untouched
            assert all(torch.equal(pool[cache.blocks("foreign")], f) for pool, f in
                       zip((pool for pools in cache._pools() for pool in pools), foreign))
        # one beam is greedy generate, with and without the eos
        assert [r[0].tokens for r in lm.beam_search(prompts, T, num_beams=1, dtype=dtype)] == free_run
        stopped = lm.generate(prompts, T, eos_token_id=eos, dtype=dtype)
        assert [r[0].tokens for r in lm.beam_search(prompts, T, num_beams=1, eos_token_id=eos, dtype=dtype)] == stopped
        # a pool that holds one prompt at a time gives the same hypotheses
        from qqq_amd import beam

        small = lm.new_cache(max(beam.blocks_needed(len(q), T, B, 16) for q in prompts), 16, dtype)
        again = lm.beam_search(prompts, T, num_beams=B, length_penalty=0.0, early_stopping=True, eos_token_id=eos, num_return_sequences=2,
                               cache=small)
        assert again == got and small.free_blocks == small.num_blocks
