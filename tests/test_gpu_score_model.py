"""QuantLlamaForCausalLM.score / loglikelihood / perplexity on the GPU against a manual loop over the same passes: pack_steps, cache.step,
lm(..., all_rows=True), and float64 log_softmax / gather / argmax of those logits on the host.  The manual loop's logits are the bits
score() sees, so the agreement is within the kernel's tolerance (tests/test_gpu_score.py) and the greedy ids are exact."""
import math

import numpy as np
import pytest
import torch

from score_ref import tolerance
from test_gpu_model import VOCAB, _make_lm, _prompts

pytestmark = pytest.mark.gpu

TOTAL = 5 + 17 + 33


def _manual(lm, seqs, chunk_tokens=2048, dtype=torch.float16):
    """-> (float64 log-probs [len - 1], int64 argmax ids [len - 1]) per sequence, from the fp16 logits of the plan's passes"""
    from qqq_amd import pack_steps

    dev = lm.lm_head.weight.device
    steps, blocks = pack_steps([len(s) for s in seqs], chunk_tokens, 16)
    cache = lm.new_cache(max(blocks), 16, dtype)
    lps, ams = [[] for _ in seqs], [[] for _ in seqs]
    with torch.no_grad():
        for step in steps:
            for i, start, _ in step:
                if start == 0:
                    cache.add(i)
            ids = torch.tensor([t for i, start, count in step for t in seqs[i][start:start + count]], dtype=torch.int64, device=dev)
            logits = lm(ids, cache, cache.step([i for i, _, _ in step], [c for _, _, c in step]), all_rows=True)
            logp = torch.log_softmax(logits.double().cpu(), -1).numpy()
            am = logits.double().cpu().numpy().argmax(1)  # numpy: the lowest index of the maximum
            row = 0
            for i, start, count in step:
                for j in range(count):
                    if start + j + 1 < len(seqs[i]):
                        lps[i].append(logp[row + j, seqs[i][start + j + 1]])
                        ams[i].append(am[row + j])
                row += count
                if start + count == len(seqs[i]):
                    cache.free(i)
    assert cache.free_blocks == max(blocks)
    return [np.array(x, np.float64) for x in lps], [np.array(x, np.int64) for x in ams]


_LMS, _REFS = {}, {}


def _lm(dev, gs):
    if gs not in _LMS:
        _LMS[gs] = _make_lm(dev, gs)
    lm = _LMS[gs]
    lm.model.unfuse_prefill()
    return lm


def _ref(dev, gs, chunk):
    """the manual log-probs of the three prompts, computed once per (group size, chunking) and shared"""
    if (gs, chunk) not in _REFS:
        _REFS[gs, chunk] = _manual(_lm(dev, gs), _prompts(), chunk)
    return _REFS[gs, chunk]


def _assert_close(got, want, what):
    err = np.abs(got.double().cpu().numpy() - want)
    print(f"{what}: max |score - manual| = {err.max():.3e}, max share of the bound = {(err / tolerance(want)).max():.3f}")
    assert (err <= tolerance(want)).all(), what


# ---- 5. score against the manual loop

@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("chunk", [64, 16])
def test_score_equals_the_manual_loop_and_frees_its_blocks(dev, gs, chunk):
    from qqq_amd import pack_steps

    lm, prompts = _lm(dev, gs), _prompts()
    assert chunk >= TOTAL or chunk == 16
    steps, blocks = pack_steps([len(p) for p in prompts], chunk, 16)
    assert len(steps) == (1 if chunk >= TOTAL else 4)  # at 16 tokens a step: splits inside and across the 5 / 17 / 33-token sequences
    want_lp, want_am = _ref(dev, gs, chunk)
    need = max(blocks)
    roomy = lm.new_cache(need + 2, 16)
    lp, am = lm.score(prompts, cache=roomy, chunk_tokens=chunk, return_greedy=True)
    assert roomy.free_blocks == need + 2 and not roomy._blocks
    for i, p in enumerate(prompts):
        assert lp[i].shape == (len(p) - 1,) and lp[i].dtype == torch.float32 and am[i].dtype == torch.int64
        _assert_close(lp[i], want_lp[i], f"gs {gs} chunk {chunk} sequence {i}")
        assert am[i].tolist() == want_am[i].tolist()
        assert torch.isfinite(lp[i]).all() and (lp[i] <= 0).all()
    # a cache of its own, and no greedy ids: the same bits
    alone = lm.score(prompts, chunk_tokens=chunk)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(alone, lp))
    # a cache that cannot hold the plan raises before anything runs and is untouched
    small = lm.new_cache(need - 1, 16)
    with pytest.raises(RuntimeError, match="score: "):
        lm.score(prompts, cache=small, chunk_tokens=chunk)
    assert small.free_blocks == need - 1 and not small._blocks
    # a single-token sequence has nothing to predict
    one = lm.score([[3], prompts[0]], chunk_tokens=chunk)
    assert one[0].shape == (0,) and one[1].shape == (4,)


# ---- 6. loglikelihood and perplexity equal their definitions

@pytest.mark.parametrize("gs", [-1, 128])
def test_loglikelihood_and_perplexity_equal_their_definitions(dev, gs):
    lm, prompts = _lm(dev, gs), _prompts()
    want_lp, want_am = _ref(dev, gs, 64)  # the requests below are the prompts, split: one pass, the logits of test 5
    cuts = (3, 9, 1)
    out = lm.loglikelihood([(p[:k], p[k:]) for p, k in zip(prompts, cuts)], chunk_tokens=64)
    for (ll, greedy), p, k, lp, am in zip(out, prompts, cuts, want_lp, want_am):
        want = float(lp[k - 1:].sum())
        assert isinstance(ll, float) and isinstance(greedy, bool)
        assert abs(ll - want) <= float(tolerance(lp[k - 1:]).sum()), (ll, want)
        assert greedy == (am[k - 1:].tolist() == p[k:])
    # a continuation that IS the greedy one, and the same with its last token changed
    k = 9
    ctx = prompts[1][:k]
    reqs = [(ctx, [int(want_am[1][k - 1])]), (ctx, [(int(want_am[1][k - 1]) + 1) % VOCAB])]
    m_lp, m_am = _manual(lm, [c + t for c, t in reqs])
    out = lm.loglikelihood(reqs)
    for (ll, greedy), lp, am, (c, t) in zip(out, m_lp, m_am, reqs):
        assert abs(ll - float(lp[-1])) <= float(tolerance(lp[-1])) and greedy == (int(am[-1]) == t[0])
    assert [g for _, g in out] == [True, False]
    # perplexity: disjoint windows of the concatenated prompts, the remainder dropped; the reference's formula on the manual log-probs
    stream, seqlen = [t for p in prompts for t in p], 16
    windows = [stream[i * seqlen:(i + 1) * seqlen] for i in range(len(stream) // seqlen)]
    assert len(windows) == 3
    w_lp, _ = _manual(lm, windows)
    nll = [float((-lp).mean()) * seqlen for lp in w_lp]
    want = math.exp(sum(nll) / (len(windows) * seqlen))
    for ids in (stream, torch.tensor(stream)[None], np.array(stream)):
        got = lm.perplexity(ids, seqlen=seqlen)
        assert abs(got - want) <= 2e-5 * want, (got, want)  # |d ln ppl| <= the mean of the per-target bounds, 8e-6 + 2^-23 * ~7
    with pytest.raises(ValueError, match="perplexity"):
        lm.perplexity(stream[:10], seqlen=16)


# ---- 7. the lossy paths run

@pytest.mark.parametrize("kind", ["int8", "fused", "int8+fused"])
def test_score_runs_on_the_int8_cache_and_the_fused_prefill(dev, kind):
    lm, prompts = _lm(dev, 128), _prompts()
    dtype = torch.int8 if "int8" in kind else torch.float16
    stream = [t for p in prompts for t in p]
    base = lm.perplexity(stream, seqlen=16)
    try:
        if "fused" in kind:
            lm.fuse_prefill()
        for chunk in (64, 16):
            cache = lm.new_cache(8, 16, dtype)
            lp = lm.score(prompts, cache=cache, chunk_tokens=chunk)
            assert cache.free_blocks == 8 and not cache._blocks
            assert all(x.shape == (len(p) - 1,) and torch.isfinite(x).all() and (x <= 0).all() for x, p in zip(lp, prompts))
        ppl = lm.perplexity(stream, seqlen=16, dtype=dtype)
    finally:
        lm.model.unfuse_prefill()
    assert math.isfinite(ppl) and ppl > 1.0
    print(f"perplexity of the toy model over 3 windows of 16 tokens: fp16 cache / SDPA prefill {base:.6f}, {kind} {ppl:.6f}, "
          f"ratio {ppl / base:.6f}")
