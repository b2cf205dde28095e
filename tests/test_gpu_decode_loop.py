"""DecodeLoop on the GPU: the eager loop against a reference loop written here from existing public pieces (a hand-built 4-row PagedStep
with idle rows, ops.sample_tokens, host bookkeeping), the captured loop against the eager one (fp16 and int8 pools, per-channel and g128,
greedy and sampled), idle rows that carry NaN, continuous batching through a pool of two budgets, and generate(device_loop=True)."""
import pytest
import torch

from test_gpu_model import LAYERS, VOCAB, _make_lm, _manual, _prompts

pytestmark = pytest.mark.gpu

ROWS, MAX_LEN, BS, N_NEW = 4, 64, 16, 8


def _blocks(prompts, n_new=N_NEW):
    return [-(-(len(p) + n_new - 1) // BS) for p in prompts]


def _reference(lm, prompts, n_new, dtype, eos=None):
    """Greedy decoding of `prompts` in rows 0 ... of a ROWS-row batch at max_len = MAX_LEN, the other rows idle at pos -1: the packed
    prefill, then lm(ids, cache, PagedStep(...)) + ops.sample_tokens per token with the bookkeeping on the host."""
    from qqq_amd import PagedStep, ops

    dev = lm.lm_head.weight.device
    cache = lm.new_cache(sum(_blocks(prompts, n_new)), BS, dtype)
    sids = list(range(len(prompts)))
    for s in sids:
        cache.add(s)
        cache.reserve(s, len(prompts[s]) + n_new - 1)
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=dev)
    logits = lm(ids, cache, cache.step(sids, [len(p) for p in prompts]))
    zero = torch.zeros(ROWS, device=dev)
    first = ops.sample_tokens(logits, 0.0, 0, 1.0, zero[:len(prompts)]).tolist()
    outs = [[t] for t in first]
    width = -(-MAX_LEN // BS)
    table = torch.zeros((ROWS, width), dtype=torch.int32)
    for s in sids:
        table[s, :len(cache.blocks(s))] = torch.tensor(cache.blocks(s), dtype=torch.int32)
    cur, pos = [0] * ROWS, [-1] * ROWS
    for s in sids:
        if n_new > 1 and first[s] != eos:
            cur[s], pos[s] = first[s], len(prompts[s])
    table_dev = table.to(dev)
    cu = torch.arange(ROWS + 1, dtype=torch.int32, device=dev)
    while any(p >= 0 for p in pos):
        slots = [-1 if p < 0 else int(table[r, p // BS]) * BS + p % BS for r, p in enumerate(pos)]
        pos_dev = torch.tensor(pos, dtype=torch.int64, device=dev)
        step = PagedStep(seq_ids=[None] * ROWS, counts=[1] * ROWS, starts=[0] * ROWS, max_len=MAX_LEN, decode=True, pos=pos_dev,
                         slots=torch.tensor(slots, dtype=torch.int64, device=dev), block_table=table_dev, last_pos=pos_dev, cu_tokens=cu,
                         start_pos=pos_dev)
        logits = lm(torch.tensor(cur, dtype=torch.int64, device=dev), cache, step)
        toks = ops.sample_tokens(logits, 0.0, 0, 1.0, zero).tolist()
        for r in range(ROWS):
            if pos[r] < 0:
                continue
            outs[r].append(toks[r])
            if len(outs[r]) >= n_new or toks[r] == eos:
                cur[r], pos[r] = 0, -1
            else:
                cur[r], pos[r] = toks[r], pos[r] + 1
    return outs


def _loop(lm, dtype, graph, num_blocks, rows=ROWS, **kw):
    from qqq_amd import DecodeLoop

    cache = lm.new_cache(num_blocks, BS, dtype)
    return DecodeLoop(lm, cache, rows=rows, max_len=MAX_LEN, sync_every=3, graph=graph, **kw), cache


@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_eager_loop_equals_the_reference_and_the_captured_loop_equals_the_eager_one(dev, dtype, gs):
    lm = _make_lm(dev, gs).fuse_prefill()
    prompts = _prompts()
    nb = sum(_blocks(prompts))
    with torch.no_grad():
        want = _reference(lm, prompts, N_NEW, dtype)
        eager, c_e = _loop(lm, dtype, False, nb)
        graph, c_g = _loop(lm, dtype, True, nb)
        got = eager.generate(prompts, N_NEW)
        assert got == want and all(len(o) == N_NEW and all(0 <= t < VOCAB for t in o) for o in got)
        assert graph.generate(prompts, N_NEW) == got
        # an eos chosen from that run: the sequence stops there, the others go on as before
        eos = want[1][2]
        stopped = _reference(lm, prompts, N_NEW, dtype, eos=eos)
        assert [o for o in stopped] == [o[:o.index(eos) + 1] if eos in o else o for o in want] and len(stopped[1]) <= 3
        assert eager.generate(prompts, N_NEW, eos_token_id=eos) == stopped == graph.generate(prompts, N_NEW, eos_token_id=eos)
        # sampled, under equally seeded generators
        runs = []
        for loop in (eager, graph):
            g = torch.Generator(device=dev).manual_seed(77)
            runs.append(loop.generate(prompts, N_NEW, temperature=0.8, top_k=50, top_p=0.9, generator=g))
        assert runs[0] == runs[1] and runs[0] != got and all(len(o) == N_NEW for o in runs[0])
        assert graph.generate(prompts, 1) == eager.generate(prompts, 1) == [o[:1] for o in want]
    assert eager.captures == 0 and graph.captures == 1
    assert c_e.free_blocks == nb and c_g.free_blocks == nb


def test_idle_rows_are_inert(dev):
    """Row 3 of the 4-row batch is idle throughout.  Its input id is set to another token and its embedding row to NaN in every decode step,
    so its q rows, its activations and its logits are NaN from the first layer on: the three active rows' tokens do not change, and nothing
    of it reaches the pool."""
    lm = _make_lm(dev, 128).fuse_prefill()
    prompts = _prompts()
    nb = sum(_blocks(prompts))

    def poison(mod, inp, out):
        if out.shape[0] != ROWS:  # the packed prefill
            return None
        out = out.clone()
        out[ROWS - 1] = float("nan")
        return out

    with torch.no_grad():
        for dtype in (torch.float16, torch.int8):
            clean, _ = _loop(lm, dtype, False, nb)
            want = clean.generate(prompts, N_NEW)
            hook = lm.model.embed_tokens.register_forward_hook(poison)
            try:
                for graph in (False, True):
                    loop, cache = _loop(lm, dtype, graph, nb)
                    loop.ids[ROWS - 1] = VOCAB - 1
                    assert loop.generate(prompts, N_NEW) == want, (dtype, graph)
                    assert loop.pos[ROWS - 1].item() == -1 and loop.n_out[ROWS - 1].item() == 0 and loop.ids[ROWS - 1].item() == VOCAB - 1
                    for l in range(LAYERS):
                        pools = (cache.k[l], cache.v[l]) + ((cache.k_scale[l], cache.v_scale[l]) if cache.quantized else ())
                        assert all(torch.isfinite(t.float()).all() for t in pools)
                    # the hook did poison the row: the idle row's logits are NaN
                    assert torch.isnan(lm(loop.ids, cache, loop.step)[ROWS - 1]).any()
            finally:
                hook.remove()


def test_continuous_batching_through_a_pool_of_two_budgets(dev):
    lm = _make_lm(dev, -1).fuse_prefill()
    g = torch.Generator().manual_seed(11)
    prompts = [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in (5, 17, 33, 9, 21)]
    assert _blocks(prompts) == [1, 2, 3, 1, 2]
    with torch.no_grad():
        loop, cache = _loop(lm, torch.float16, True, 5, rows=2)  # the two largest budgets, and never three of the five
        got = loop.generate(prompts, N_NEW)
        assert all(len(o) == N_NEW for o in got) and cache.free_blocks == 5
        for p, o in zip(prompts, got):
            assert loop.generate([p], N_NEW) == [o]
        assert loop.captures == 1 and cache.free_blocks == 5
        eager, c_e = _loop(lm, torch.float16, False, 5, rows=2)
        assert eager.generate(prompts, N_NEW) == got and c_e.free_blocks == 5
        # a pool that cannot hold the largest budget: the loop says so and leaves the pool as it found it
        small, c_s = _loop(lm, torch.float16, False, 4, rows=2)
        c_s.add("other")
        c_s.reserve("other", 2 * BS)
        with pytest.raises(RuntimeError, match="cannot hold a prompt"):
            small.generate(prompts[2:3], N_NEW)
        assert c_s.free_blocks == 2


def test_generate_device_loop_is_the_decode_loop_and_the_default_path_is_unchanged(dev):
    from qqq_amd import DecodeLoop

    lm = _make_lm(dev, 128).fuse_prefill()
    prompts = _prompts()
    need = _blocks(prompts)
    with torch.no_grad():
        cache = lm.new_cache(sum(need), BS)
        want = DecodeLoop(lm, cache, rows=len(prompts), max_len=max(need) * BS).generate(prompts, N_NEW)
        assert lm.generate(prompts, N_NEW, device_loop=True) == want
        assert lm.generate(prompts, N_NEW, device_loop=True, cache=cache) == want and cache.free_blocks == sum(need)
        g1, g2 = (torch.Generator(device=dev).manual_seed(5) for _ in range(2))
        sampled = lm.generate(prompts, N_NEW, temperature=0.8, top_k=50, top_p=0.9, generator=g1, device_loop=True)
        assert sampled == DecodeLoop(lm, cache, rows=len(prompts), max_len=max(need) * BS).generate(
            prompts, N_NEW, temperature=0.8, top_k=50, top_p=0.9, generator=g2)
        # the default path: what tests/test_gpu_model.py holds it to
        assert lm.generate(prompts, N_NEW) == _manual(lm, prompts, N_NEW, 0.0, 0, 1.0, 0)


def test_a_prompt_beyond_max_len_raises_before_anything_runs(dev):
    lm = _make_lm(dev, -1)
    loop, cache = _loop(lm, torch.float16, True, 8)
    with pytest.raises(ValueError, match="max_len=64"):
        loop.generate([[1] * 5, [2] * 60], 6)  # 60 + 6 - 1 = 65 keys
    assert loop.captures == 0 and cache.free_blocks == 8 and loop.generate([[1] * 5], 0) == [[]]
    from qqq_amd import DecodeLoop

    with pytest.raises(ValueError, match="u_stride"):
        DecodeLoop(lm, cache, rows=2, max_len=64, sync_every=8, u_stride=4)
    with pytest.raises(ValueError, match="exceeds what the pool could hold"):
        DecodeLoop(lm, cache, rows=2, max_len=8 * BS + 1)
