"""generate(..., n=N) on the GPU: N completions per prompt over forked sequences, on the host path and in DecodeLoop(family=N), with
fuse_shared() on and off.  Greedy completions against the n = 1 call, sampled ones between equally seeded runs and between the two
attention routes, eos and budgets per sibling, the pool's blocks against the arithmetic of the family budget, admission into slots, and
the refusals.  One prompt is longer than a 128-key chunk of the decode plan, so its siblings' steps contain a jointly taken split."""
import pytest
import torch

from test_gpu_model import VOCAB, _make_lm

pytestmark = pytest.mark.gpu

BS = 16
LENS = (5, 16, 37, 140)  # inside a block, exactly a block, two blocks and a part, and 128 shared keys: one whole chunk


def _prompts(lens=LENS, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in lens]


def _need(prompts, n_new):
    return [-(-(len(p) + n_new - 1) // BS) for p in prompts]


def _family_blocks(prompts, n_new, n):
    """the prompt's budget once plus, per further sibling, the blocks beyond the prompt's full ones"""
    return [nd + (n - 1) * (nd - len(p) // BS) for nd, p in zip(_need(prompts, n_new), prompts)]


def _watch(cache):
    """record the fewest free blocks seen after any call that takes blocks"""
    low = [cache.free_blocks]
    for name in ("step", "reserve", "fork"):
        def wrapped(*a, _f=getattr(cache, name), **kw):
            out = _f(*a, **kw)
            low[0] = min(low[0], cache.free_blocks)
            return out
        setattr(cache, name, wrapped)
    return low


def _run(lm, prompts, n_new, n, dtype, path, spare=0, gen=None, **kw):
    """path: 'host', 'graph' (generate(device_loop=True)) or 'eager' (a DecodeLoop with graph=False) -> (completions, peak blocks in use)"""
    from qqq_amd.serve import DecodeLoop

    cache = lm.new_cache(sum(_family_blocks(prompts, n_new, n)) + spare, BS, dtype)
    low = _watch(cache)
    if gen is not None:
        kw["generator"] = torch.Generator(device=lm.lm_head.weight.device).manual_seed(gen)
    if path == "eager":
        extra = dict(penalties=True) if "repetition_penalty" in kw else {}
        loop = DecodeLoop(lm, cache, rows=len(prompts) * n, max_len=max(_need(prompts, n_new)) * BS, graph=False, family=n, **extra)
        out = loop.generate(prompts, n_new, **kw)
    else:
        out = lm.generate(prompts, n_new, cache=cache, n=n, device_loop=path == "graph", **kw)
    assert cache.free_blocks == cache.num_blocks  # every block is free again, the shared ones included
    return out, cache.num_blocks - low[0]


@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_greedy_siblings_equal_the_single_completion(dev, dtype, gs):
    lm = _make_lm(dev, gs).fuse_prefill()
    prompts, n_new = _prompts(), 7
    want, _ = _run(lm, prompts, n_new, 1, dtype, "host")
    assert all(len(w) == n_new for w in want)
    for fused in (False, True):
        lm.fuse_shared() if fused else lm.unfuse_shared()
        for path in ("host", "graph", "eager"):
            got, _ = _run(lm, prompts, n_new, 3, dtype, path)
            assert len(got) == len(prompts)
            for comps, w in zip(got, want):
                assert len(comps) == 3
                for c in comps:
                    assert c == w, (fused, path)


@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
@pytest.mark.parametrize("path", ["host", "graph"])
def test_sampled_siblings_are_reproducible_distinct_and_the_same_on_both_routes(dev, dtype, gs, path):
    lm = _make_lm(dev, gs).fuse_prefill()
    prompts, n_new, n = _prompts(), 12, 4
    kw = dict(temperature=0.8, top_k=50, top_p=0.9)
    if dtype == torch.int8 and gs == 128:  # penalties in one case
        kw.update(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1)
    plain, _ = _run(lm.unfuse_shared(), prompts, n_new, n, dtype, path, gen=17, **kw)
    fused, _ = _run(lm.fuse_shared(), prompts, n_new, n, dtype, path, gen=17, **kw)
    again, _ = _run(lm, prompts, n_new, n, dtype, path, gen=17, **kw)
    assert fused == plain and again == fused
    for comps in fused:
        assert len(comps) == n and all(len(c) == n_new for c in comps)
        assert len({tuple(c) for c in comps}) == n  # every sibling drew its own variates
    other, _ = _run(lm, prompts, n_new, n, dtype, path, gen=18, **kw)
    assert other != fused


@pytest.mark.parametrize("path", ["host", "graph"])
def test_a_sibling_that_ends_at_once_and_one_that_runs_to_the_budget(dev, path):
    lm = _make_lm(dev, 128).fuse_prefill().fuse_shared()
    prompts, n_new, n = _prompts(), 9, 4
    kw = dict(temperature=0.8, top_k=50, top_p=0.9)
    free, _ = _run(lm, prompts, n_new, n, torch.float16, path, gen=5, **kw)
    firsts = [c[0] for c in free[3]]  # the first draws do not depend on eos: the same variates over the same logits
    assert len(set(firsts)) > 1
    eos = firsts[1]
    got, _ = _run(lm, prompts, n_new, n, torch.float16, path, gen=5, eos_token_id=eos, **kw)
    assert [c[0] for c in got[3]] == firsts
    assert got[3][1] == [eos]  # ended at its first token, while its siblings were forked and went on
    flat = [c for comps in got for c in comps]
    assert any(len(c) == n_new and eos not in c for c in flat)  # another one ran to the budget
    for c in flat:
        assert len(c) <= n_new and eos not in c[:-1] and (c[-1] == eos or len(c) == n_new)


@pytest.mark.parametrize("path", ["host", "graph"])
def test_peak_blocks_are_the_family_budget(dev, path):
    lm = _make_lm(dev, -1).fuse_prefill().fuse_shared()
    prompts, n_new, n = _prompts((5, 16, 37)), 8, 3
    assert _need(prompts, n_new) == [1, 2, 3] and _family_blocks(prompts, n_new, n) == [3, 4, 5]
    _, peak = _run(lm, prompts, n_new, n, torch.float16, path, spare=9)
    assert peak == 12 < n * 6  # n separate prompts would take 18


def test_more_prompts_than_slots_are_admitted_as_slots_free_up(dev):
    from qqq_amd.serve import DecodeLoop

    lm = _make_lm(dev, 128).fuse_prefill().fuse_shared()
    prompts, n = _prompts((5, 16, 37, 9, 21)), 3
    budgets = 6
    want, _ = _run(lm, prompts, budgets, 1, torch.float16, "host")
    cache = lm.new_cache(64, BS)
    loop = DecodeLoop(lm, cache, rows=2 * n, max_len=64, sync_every=2, family=n)  # two slots for five prompts
    got = loop.generate(prompts, budgets)
    assert cache.free_blocks == cache.num_blocks and loop.captures == 1
    assert got == [[w] * n for w in want]
    assert int(loop.shared.abs().sum()) == 0 and loop.family_of.tolist() == [0, 0, 0, 3, 3, 3]
    # a pool that holds one family at a time serves them one after the other
    small = lm.new_cache(max(_family_blocks(prompts, budgets, n)), BS)
    assert lm.generate(prompts, budgets, cache=small, n=n) == got and small.free_blocks == small.num_blocks


def test_refusals(dev):
    from qqq_amd.serve import DecodeLoop, SpecDecodeLoop

    lm = _make_lm(dev, -1).fuse_prefill()
    cache = lm.new_cache(32, BS)
    with pytest.raises(ValueError, match="n=0"):
        lm.generate(_prompts(), 4, n=0)
    with pytest.raises(ValueError, match="family"):
        DecodeLoop(lm, cache, rows=4, max_len=64, family=3)
    with pytest.raises(ValueError, match="family"):
        SpecDecodeLoop(lm, cache, rows=4, max_len=64, draft_len=2, family=2)
    with pytest.raises(ValueError, match="draft_len"):
        lm.generate(_prompts(), 4, n=2, draft_len=2, device_loop=True)
    assert cache.free_blocks == cache.num_blocks
