"""ops.beam_step and ops.copy_blocks on the GPU.

beam_step against tests/beam_ref.py, bit for bit: rule 1 of include/qqq_amd_beam.h defines a row's candidates as ops.topk_logprobs'
(ids exactly, values to the bit), so the reference merge runs on that op's output for the same logits -- f32 arithmetic that numpy repeats
exactly -- and every output of beam_step is compared as a bit pattern.  The candidates' ids are checked against the float64 reference of
the order as well.  copy_blocks byte for byte against torch indexing."""
import numpy as np
import pytest
import torch

import beam_ref
import logprobs_ref

pytestmark = pytest.mark.gpu

OUT = ("cand_score", "cand_logprob", "cand_parent", "cand_token", "next_ids", "next_parent", "next_cum", "next_live")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _inputs(P, B, vocab, seed):
    """logits fp16 [P * B, vocab], cum f32, live int32 with, where the shape has room: two identical rows with one cum (prompt 0, beams 0
    and 1), a row with far more than 2B tokens tied at its cut (beam 2), a row with two logits above -inf (beam 3), a row with none (beam
    4), a dead row among live ones (beam 5); in prompt 1 beam 0 a thousand nats ahead of the others, whose last one has no logit above
    -inf; prompt 2 without a live row."""
    rng = np.random.default_rng(seed)
    rows = P * B
    logits = (rng.standard_normal((rows, vocab)) * 3).astype(np.float16)
    cum = (-rng.random(rows) * 4).astype(np.float32)
    live = np.ones(rows, np.int32)
    if B >= 2:
        logits[1] = logits[0]
        cum[0] = cum[1] = 5.0  # ahead of every other beam: the pair's candidates lead the prompt's list
    if B >= 4:
        logits[2] = 0.0
        logits[2, rng.choice(vocab, 3, replace=False)] = 1.0
        logits[3] = -np.inf
        logits[3, [vocab - 1, vocab // 2]] = [2.0, 2.5]
    if B >= 16:
        logits[4] = -np.inf
        logits[5], live[5] = np.inf, 0
    if B == 1:
        logits[0, 7], logits[0, 3] = 9.0, 9.0  # a tie at the very top
    if P >= 3:
        cum[B:2 * B] = -1000.0
        cum[B] = 0.0
        if B >= 2:
            logits[2 * B - 1] = -np.inf
        else:
            logits[B] = -np.inf
            logits[B, vocab - 2] = 1.0
        logits[2 * B:3 * B], live[2 * B:3 * B] = np.nan, 0
    return logits, cum, live


def _on(dev, logits, ld):
    wide = torch.full((logits.shape[0], ld), float("nan"), dtype=torch.float16, device=dev)
    wide[:, :logits.shape[1]] = torch.from_numpy(logits).to(dev)
    return wide[:, :logits.shape[1]]


def _want(dev, view, cum, live, B, eos):
    """the reference merge over ops.topk_logprobs' candidates of the same rows"""
    from qqq_amd import ops

    _, _, ids, lps = ops.topk_logprobs(view, None, 2 * B)
    return beam_ref.merge(ids.cpu().numpy(), lps.cpu().numpy(), cum, live, B, eos), ids.cpu().numpy()


def _got(step):
    return {name: getattr(step, name).cpu().numpy() for name in OUT}


def _assert_same(got, want, live, B, note):
    for name in OUT:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (note, name)
        assert np.array_equal(_bits(got[name]), _bits(want[name])), (note, name, got[name], want[name])


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("B", [1, 4, 16])
@pytest.mark.parametrize("vocab, ld", [(32, 40), (1000, 1024), (32003, 32008)])
def test_beam_step_equals_the_reference_bit_for_bit(dev, vocab, ld, B, P):
    from qqq_amd import ops

    logits, cum, live = _inputs(P, B, vocab, seed=vocab + 17 * B + P)
    view = _on(dev, logits, ld)
    c, l = torch.from_numpy(cum).to(dev), torch.from_numpy(live).to(dev)
    ws = ops.beam_step_workspace(P * B, B, dev)
    plain, ids = _want(dev, view, cum, live, B, -1)
    for r in range(P * B):  # rule 1's ids against the float64 reference of the order
        if live[r]:
            assert np.array_equal(ids[r], logprobs_ref.order(logits[r])[:2 * B]), r
    inside, outside = int(plain["cand_token"][0, 0]), int(plain["cand_token"][0, 2 * B - 1])
    for eos in (-1, inside, outside):  # eos among the first B candidates of prompt 0, and behind them
        step = ops.beam_step(view, c, l, B, eos, ws)
        torch.cuda.synchronize()
        want = _want(dev, view, cum, live, B, eos)[0]
        _assert_same(_got(step), want, live, B, (vocab, B, P, eos))
        assert torch.equal(step.packed[:2 * P * B].view(torch.float32).view(P, 2 * B), step.cand_score)  # the views are the packed block's
    got = _got(ops.beam_step(view, c, l, B, inside))  # without a workspace of the caller's
    _assert_same(got, _want(dev, view, cum, live, B, inside)[0], live, B, "own workspace")
    # what the inputs were made for
    if B >= 2:
        pair = [(b, t) for b, t in zip(plain["cand_parent"][0].tolist(), plain["cand_token"][0].tolist()) if b in (0, 1)]
        mine = [[t for b, t in pair if b == which] for which in (0, 1)]
        assert len(mine[1]) >= 1 and mine[0][:len(mine[1])] == mine[1]  # the tie: both beams' candidates, in one order ...
        assert all(sum(b == 0 for b, _ in pair[:n]) >= sum(b == 1 for b, _ in pair[:n]) for n in range(len(pair) + 1))  # ... the lower beam first
    if P >= 3:
        assert (plain["cand_parent"][1] == 0).all() and (plain["cand_parent"][2] == -1).all() and (plain["next_live"][2 * B:] == 0).all()
        assert np.isneginf(plain["cand_score"][2]).all() and (plain["next_live"][:2 * B] == 1).all()
    assert inside not in got["next_ids"][:B].tolist()  # an eos never goes on


def test_a_prompt_gives_the_same_bits_at_any_index_and_row_stride(dev):
    from qqq_amd import ops

    B, vocab = 4, 1000
    logits, cum, live = _inputs(1, B, vocab, seed=5)
    other = _inputs(1, B, vocab, seed=6)
    three = np.concatenate([logits, other[0], logits]), np.concatenate([cum, other[1], cum]), np.concatenate([live, other[2], live])
    eos = int(np.argmax(logits[0].astype(np.float32)))
    a = _got(ops.beam_step(_on(dev, three[0], 1000), torch.from_numpy(three[1]).to(dev), torch.from_numpy(three[2]).to(dev), B, eos))
    b = _got(ops.beam_step(_on(dev, logits, 1048), torch.from_numpy(cum).to(dev), torch.from_numpy(live).to(dev), B, eos))
    for name in OUT:
        per = 2 * B if name.startswith("cand") else B
        x = a[name].reshape(3, per)
        assert np.array_equal(_bits(x[0]), _bits(x[2])) and np.array_equal(_bits(x[0]), _bits(b[name].reshape(1, per)[0])), name
    assert not np.array_equal(_bits(a["cand_score"][0]), _bits(a["cand_score"][1]))  # the prompt between them is another one


def test_hipgraph_replays_with_new_contents(dev):
    from qqq_amd import ops

    P, B, vocab = 3, 4, 4099
    logits = torch.zeros((P * B, vocab + 5), dtype=torch.float16, device=dev)[:, :vocab]
    cum = torch.zeros(P * B, device=dev)
    live = torch.ones(P * B, dtype=torch.int32, device=dev)
    ws = ops.beam_step_workspace(P * B, B, dev)

    def fill(i):
        a, c, l = _inputs(P, B, vocab, seed=100 + i)
        logits.copy_(torch.from_numpy(a).to(dev))
        cum.copy_(torch.from_numpy(c).to(dev))
        live.copy_(torch.from_numpy(np.roll(l, i * B)).to(dev))  # the dead prompt moves

    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.beam_step(logits, cum, live, B, 11, ws)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = ops.beam_step(logits, cum, live, B, 11, ws)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for i in range(1, 4):
        fill(i)
        graph.replay()
        torch.cuda.synchronize()
        replayed = _got(out)
        eager = _got(ops.beam_step(logits, cum, live, B, 11))
        for name in OUT:
            assert np.array_equal(_bits(replayed[name]), _bits(eager[name])), (i, name)
        seen.append(replayed["cand_token"].tobytes())
    assert len(set(seen)) == 3


# ---- copy_blocks

@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
@pytest.mark.parametrize("layers, bs, d", [(1, 16, 64), (3, 16, 128), (1, 256, 64), (3, 256, 128)])
def test_copy_blocks_is_byte_exact_and_touches_nothing_else(dev, dtype, layers, bs, d):
    from qqq_amd import PagedKVCache, ops

    nb, kvh = 12, 2
    cache = PagedKVCache(layers, nb, kvh, d, bs, device=dev, dtype=dtype)
    g = torch.Generator(device=dev).manual_seed(layers * bs + d)
    for pools in cache._pools():
        for pool in pools:
            if pool.dtype == torch.int8:
                pool.copy_(torch.randint(-128, 128, pool.shape, generator=g, device=dev, dtype=torch.int8))
            else:
                pool.copy_(torch.randn(pool.shape, generator=g, device=dev).to(pool.dtype))
    before = [[pool.clone() for pool in pools] for pools in cache._pools()]
    src, dst = [5, 5, 5, 0, 11], [1, 7, 9, 10, 2]  # one source to three destinations, the pool's first and last block
    s, t = (torch.tensor(x, dtype=torch.int32, device=dev) for x in (src, dst))
    tables = cache._pool_tables()
    assert len(tables) == (2 if dtype == torch.int8 else 1) and tables[0][0].shape[0] == 2 * layers
    assert tables[0][1] == kvh * bs * d * (1 if dtype == torch.int8 else 2) and cache._pool_tables() is tables  # built once per cache
    for table, block_bytes in tables:
        ops.copy_blocks(table, s[:0], t[:0], block_bytes, nb)  # n = 0: nothing
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for pa, pb in zip(before, cache._pools()) for a, b in zip(pa, pb))
    for table, block_bytes in tables:
        ops.copy_blocks(table, s, t, block_bytes, nb)
    torch.cuda.synchronize()
    for olds, news in zip(before, cache._pools()):
        for old, new in zip(olds, news):
            want = old.clone()
            want[dst] = old[src]
            assert torch.equal(new.view(torch.uint8), want.view(torch.uint8))
    # ids outside the pool copy nothing
    ops.copy_blocks(tables[0][0], torch.tensor([nb, -1, 3], dtype=torch.int32, device=dev), torch.tensor([4, 6, nb], dtype=torch.int32, device=dev),
                    tables[0][1], nb)
    torch.cuda.synchronize()
    assert torch.equal(cache.k[0][[4, 6]], before[0][0][[4, 6]])


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_reorder_on_gpu_pools_goes_through_copy_blocks(dev, dtype, monkeypatch):
    from qqq_amd import PagedKVCache, ops

    cache = PagedKVCache(2, 16, 2, 64, 16, device=dev, dtype=dtype)
    g = torch.Generator(device=dev).manual_seed(3)
    for pools in cache._pools():
        for pool in pools:
            pool.copy_((torch.randn(pool.shape, generator=g, device=dev) * 20).to(pool.dtype))
    for s in range(3):
        cache.add(s)
    cache.step([0, 1, 2], [21, 21, 21])
    want = [x.clone() for x in cache.gather(1, 1)]
    calls = []
    real = ops.copy_blocks
    monkeypatch.setattr(ops, "copy_blocks", lambda *a: (calls.append(a[1].shape[0]), real(*a))[1])
    cache.reorder([0, 1, 2, 3], [1, 1, 2, 1])
    torch.cuda.synchronize()
    assert calls == ([2, 2] if dtype == torch.int8 else [2])  # two copies of the partial block, one launch per pool table
    for s in (0, 1, 3):
        assert all(torch.equal(a, b) for a, b in zip(cache.gather(1, s), want))
        assert cache.blocks(s)[0] == cache.blocks(0)[0] and cache.shared_keys(s) == 16
    assert len({cache.blocks(s)[1] for s in range(4)}) == 4
    for s in range(4):
        cache.free(s)
    assert cache.free_blocks == 16
