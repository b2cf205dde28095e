"""The verify chunk's attention on the GPU (include/qqq_amd_verify.h): every token of a chunk bit for bit the decode op's for that token
alone (equal b, kvh and max_len, pos = start + j), tokens and rows that write nothing, one float64 check per pool dtype, hipGraph replay with
every input updated in place, the layer stack of a verify step against successive decode steps, and SpecDecodeLoop with fuse_verify().

block_size 16, max_len 640 and kvh <= 4 throughout the op tests: the split plan is then the bound of one split per 128 keys, five splits."""
import pytest
import torch

import kv8_ref as K8
from test_gpu_decode_attn import _chunk, _errors, _ref64
from test_gpu_paged import SENT, _decode_case, _from_pool, _i32, _raw

pytestmark = pytest.mark.gpu

BS, MAX_LEN, B = 16, 640, 4
CASES = [(4, 4, 5), (4, 4, 16), (8, 2, 5), (28, 4, 3), (6, 2, 16), (16, 2, 8), (8, 2, 1)]


def _poisoned_chunk(table, start, t, bs, poison, max_len):
    """int32 table whose entries beyond each row's last block ((start + t - 1) // bs, below max_len) name the poison block"""
    last = ((start + t - 1).clamp(0, max_len - 1) // bs)[:, None]
    cols = torch.arange(table.shape[1], device=table.device)[None]
    return torch.where(cols <= last, table, torch.full_like(table, poison)).to(torch.int32)


def _verify(q, pools, table, start, t, scale, max_len, kv8):
    from qqq_amd import ops

    op = ops.verify_attention_paged_kv8 if kv8 else ops.verify_attention_paged
    return op(q, *pools, table, start, t, scale, max_len=max_len, return_fp16=True)


def _decode(q, pools, table, pos, scale, max_len, kv8):
    from qqq_amd import ops

    op = ops.decode_attention_paged_kv8 if kv8 else ops.decode_attention_paged
    return op(q, *pools, table, pos, scale, max_len=max_len, return_fp16=True)


def _assert_tokens_equal_decode(got, q, pools, table, start, t, scale, max_len, kv8, what, rows=None):
    """token j of every row in `rows` (default: all) against the decode op at the same b with pos = start + j"""
    b = start.numel()
    got = [x.reshape(b, t, -1) for x in got]
    q4 = q.reshape(b, t, q.shape[1], q.shape[2])
    for j in range(t):
        pos = start + j
        want = _decode(q4[:, j].contiguous(), pools, table, pos, scale, max_len, kv8)
        for r in range(b) if rows is None else rows:
            if not 0 <= int(pos[r]) < max_len:
                continue
            for name, g_, w_ in zip(("xq", "s1", "o_fp16"), got, want):
                assert torch.isfinite(g_[r, j].float()).all(), (what, name, r, j)
                assert torch.equal(_raw(g_[r, j]), _raw(w_[r])), (what, name, r, j)


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,kvh,t", CASES)
def test_every_token_equals_the_decode_op(dev, h, kvh, t, d, kv8):
    g = torch.Generator(device=dev).manual_seed(h * 11 + kvh + t * 3 + d)
    assert _chunk(dev, B, kvh, MAX_LEN) == 128  # the plan of the docstring
    _, pools, table, poison = _decode_case(dev, g, B, h, kvh, d, MAX_LEN, BS, kv8)
    q = torch.randn((B * t, h, d), generator=g, device=dev).half()
    start = torch.tensor((0, 30, 126, MAX_LEN - t), dtype=torch.int64, device=dev)
    tab = _poisoned_chunk(table, start, t, BS, poison, MAX_LEN)
    got = _verify(q, pools, tab, start, t, d ** -0.5, MAX_LEN, kv8)
    assert got[0].shape == (B * t, h * d) and got[1].shape == (B * t, 1) and got[2].shape == (B * t, h * d)
    # the decode calls read the table up to their own position only: the chunk's table serves them
    _assert_tokens_equal_decode(got, q, pools, tab, start, t, d ** -0.5, MAX_LEN, kv8, (h, kvh, t, d, kv8))
    # o_fp16 = None and xq / s1 = None are the same numbers
    from qqq_amd import ops

    op = ops.verify_attention_paged_kv8 if kv8 else ops.verify_attention_paged
    xq, s1 = op(q, *pools, tab, start, t, d ** -0.5, max_len=MAX_LEN)
    assert torch.equal(xq, got[0]) and torch.equal(_i32(s1), _i32(got[1]))


@pytest.mark.parametrize("kv8", [False, True])
def test_rows_and_tokens_out_of_range_write_nothing(dev, kv8):
    from qqq_amd import _lib

    h, kvh, d, t, b = 8, 2, 128, 5, 4
    g = torch.Generator(device=dev).manual_seed(29)
    _, pools, table, poison = _decode_case(dev, g, b, h, kvh, d, MAX_LEN, BS, kv8)
    saved = [x.clone() for x in pools]
    q = torch.randn((b * t, h, d), generator=g, device=dev).half()
    start = torch.tensor([-1, MAX_LEN - 2, 200, MAX_LEN], dtype=torch.int64, device=dev)  # row 1: tokens 0 and 1 are below max_len
    tab = _poisoned_chunk(table, start, t, BS, poison, MAX_LEN)
    tab[0], tab[3] = -7, 1 << 30  # rows that are never read
    tab[2, 204 // BS + 1:] = 1 << 30  # beyond the block of row 2's last key: out-of-pool ids that are never read
    o = torch.full((b * t, h * d), SENT, dtype=torch.float16, device=dev)
    xq = torch.full((b * t, h * d), 77, dtype=torch.int8, device=dev)
    s1 = torch.full((b * t, 1), SENT, dtype=torch.float32, device=dev)
    L = _lib.lib()
    nbytes = L.qqq_verify_attn_workspace_bytes(b, t, h, kvh, d, MAX_LEN)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    tail = (tab.data_ptr(), tab.shape[1], start.data_ptr(), d ** -0.5, o.data_ptr(), xq.data_ptr(), s1.data_ptr(), ws.data_ptr(), nbytes, b, t,
            h, kvh, d, pools[0].shape[0], BS, MAX_LEN, 0, torch.cuda.current_stream().cuda_stream)
    fn = L.qqq_verify_attn_paged_kv8 if kv8 else L.qqq_verify_attn_paged
    err = fn(q.data_ptr(), *(x.data_ptr() for x in pools), *tail)
    torch.cuda.synchronize()
    assert err == 0, _lib.last_error()
    untouched = [0 * t + j for j in range(t)] + [1 * t + j for j in range(2, t)] + [3 * t + j for j in range(t)]
    for row in untouched:
        assert bool((o[row] == SENT).all()) and bool((xq[row] == 77).all()) and float(s1[row]) == SENT, row
    for x, x0 in zip(pools, saved):
        assert torch.equal(_raw(x), _raw(x0))  # the pools are only read
    # rows 1 (its two tokens below max_len) and 2 against the decode op; the decode calls get a table without the out-of-pool ids of
    # rows 0 and 3, which they would not read either
    _assert_tokens_equal_decode((xq, s1, o), q, pools, tab, start, t, d ** -0.5, MAX_LEN, kv8, "partial rows", rows=(1, 2))
    assert bool((o[1 * t + 1] != SENT).any()) and bool((o[2 * t + 4] != SENT).any())


@pytest.mark.parametrize("kv8", [False, True])
def test_verify_attention_paged_against_float64(dev, kv8):
    """The absolute anchor: relative L2 per (token, head) <= 1e-3 and max error <= 2^-9 max|v|, the bounds and the float64 reference of
    tests/test_gpu_paged.py::test_decode_attention_paged_against_float64."""
    h, kvh, d, b, cap, bs, t = 32, 8, 128, 3, 4224, 16, 5
    g = torch.Generator(device=dev).manual_seed(31)
    _, pools, table, poison = _decode_case(dev, g, b, h, kvh, d, cap, bs, kv8)
    q = torch.randn((b * t, h, d), generator=g, device=dev).half()
    start = torch.tensor((17, 2077, cap - t), dtype=torch.int64, device=dev)
    got = _verify(q, pools, _poisoned_chunk(table, start, t, bs, poison, cap), start, t, d ** -0.5, cap, kv8)
    if kv8:
        k64, v64 = K8.dequant64(_from_pool(pools[0], table), _from_pool(pools[2], table)), K8.dequant64(_from_pool(pools[1], table),
                                                                                                      _from_pool(pools[3], table))
    else:
        k64, v64 = _from_pool(pools[0], table), _from_pool(pools[1], table)
    o = got[2].reshape(b, t, h * d)
    q4 = q.reshape(b, t, h, d)
    worst = (0.0, 0.0)
    for j in range(t):
        pos = start + j
        qj = q4[:, j, :, None].contiguous()
        ref = K8.attention64(qj, k64, v64, pos, d ** -0.5) if kv8 else _ref64(qj, k64, v64, pos, d ** -0.5)
        rel, mx = _errors(o[:, j].contiguous(), ref, v64, pos)
        worst = (max(worst[0], rel), max(worst[1], mx))
    print(f"verify_attention_paged{'_kv8' if kv8 else ''} vs float64: rel L2 {worst[0]:.2e}, max|err|/max|v| {worst[1]:.2e} "
          f"(2^-9 = {2 ** -9:.2e})")
    assert worst[0] <= 1e-3 and worst[1] <= 2 ** -9, worst


@pytest.mark.parametrize("kv8", [False, True])
def test_hipgraph_replays_with_every_input_updated_in_place(dev, kv8):
    h, kvh, d, b, t = 8, 2, 128, 3, 4
    g = torch.Generator(device=dev).manual_seed(43)
    _, pools, table, poison = _decode_case(dev, g, b, h, kvh, d, MAX_LEN, BS, kv8)
    q = torch.randn((b * t, h, d), generator=g, device=dev).half()
    start = torch.tensor((3, 100, 500), dtype=torch.int64, device=dev)
    tab = _poisoned_chunk(table, start, t, BS, poison, MAX_LEN)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _verify(q, pools, tab, start, t, d ** -0.5, MAX_LEN, kv8)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = _verify(q, pools, tab, start, t, d ** -0.5, MAX_LEN, kv8)
    torch.cuda.current_stream().wait_stream(side)
    first = [x.clone() for x in out]
    # other contents of everything: positions in other splits (one row out of range), other queries, another table, other pool rows
    _, pools2, table2, poison2 = _decode_case(dev, g, b, h, kvh, d, MAX_LEN, BS, kv8)
    start2 = torch.tensor((MAX_LEN - t, -1, 127), dtype=torch.int64, device=dev)
    for x, x2 in zip(pools, pools2):
        x.copy_(x2)
    start.copy_(start2)
    q.copy_(torch.randn(q.shape, generator=g, device=dev).half())
    tab.copy_(_poisoned_chunk(table2, start2, t, BS, poison2, MAX_LEN))
    graph.replay()
    torch.cuda.synchronize()
    want = _verify(q, pools, tab, start, t, d ** -0.5, MAX_LEN, kv8)
    live = [r * t + j for r in (0, 2) for j in range(t)]
    for g_, w_, f_ in zip(out, want, first):
        assert torch.equal(_raw(g_[live]), _raw(w_[live]))
        assert not torch.equal(_raw(g_[live]), _raw(f_[live]))
    _assert_tokens_equal_decode(out, q, pools, tab, start, t, d ** -0.5, MAX_LEN, kv8, "replay", rows=(0, 2))


# ---- the layer stack and the loop

def _lm(dev, gs, flag):
    from test_gpu_spec_loop import _make_lm

    lm = _make_lm(dev, gs)  # comes with fuse_prefill()
    if flag == "verify":
        lm.model.unfuse_prefill()
        lm.fuse_verify()
    return lm


@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_a_verify_step_equals_successive_decode_steps(dev, dtype, gs, monkeypatch):
    from qqq_amd import ops
    from test_gpu_spec_loop import VOCAB

    R, T, max_len = 2, 4, 64
    lens = (9, 30)  # the second row's chunk crosses a 32-key block
    gen = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, VOCAB, (n,), generator=gen).tolist() for n in lens]
    chunk = torch.randint(0, VOCAB, (R, T), generator=gen)
    calls = []
    for name in ("verify_attention_paged", "verify_attention_paged_kv8", "prefill_attention_paged", "prefill_attention_paged_kv8"):
        real = getattr(ops, name)
        monkeypatch.setattr(f"qqq_amd.attention.ops.{name}", lambda *a, _n=name, _f=real, **kw: (calls.append(_n), _f(*a, **kw))[1])

    def caches(lm):
        cache = lm.new_cache(2 * (max_len // BS), BS, dtype)
        for s in range(R):
            cache.add(s)
            cache.reserve(s, max_len)
        ids = torch.tensor([x for p in prompts for x in p], dtype=torch.int64, device=dev)
        lm.model(ids, cache, cache.step(list(range(R)), list(lens)))
        return cache

    with torch.no_grad():
        lm = _lm(dev, gs, "verify")
        # the decode steps, teacher-forced with the chunk's tokens, over a cache of their own
        cache = caches(lm)
        calls.clear()
        want = []
        for j in range(T):
            step = cache.step(list(range(R)), [1] * R)
            assert step.decode and step.max_len <= max_len
            step.max_len = max_len  # the verify step's launch is sized for max_len: the same split plan
            want.append(lm.model(chunk[:, j].to(dev), cache, step, all_rows=True))
        assert calls == []
        want = torch.stack(want, 1).reshape(R * T, -1)
        cache = caches(lm)
        calls.clear()
        step = cache.step(list(range(R)), [T] * R)
        step.max_len = max_len
        got = lm.model(chunk.reshape(-1).to(dev), cache, step, all_rows=True)
        name = "verify_attention_paged" + ("_kv8" if dtype == torch.int8 else "")
        assert calls == [name] * len(lm.model.layers)
        assert torch.isfinite(got.float()).all() and torch.equal(_raw(got), _raw(want))
        # with fuse_prefill() instead, the chunk goes where it went before
        lm = _lm(dev, gs, "prefill")
        cache = caches(lm)
        calls.clear()
        step = cache.step(list(range(R)), [T] * R)
        lm.model(chunk.reshape(-1).to(dev), cache, step, all_rows=True)
        assert calls == [name.replace("verify", "prefill")] * len(lm.model.layers)


def _spec_loop(lm, dtype, graph, num_blocks, rows):
    from qqq_amd import SpecDecodeLoop
    from test_gpu_spec_loop import K, MAX_LEN as LOOP_MAX_LEN, NGRAM, SYNC

    cache = lm.new_cache(num_blocks, BS, dtype)
    return SpecDecodeLoop(lm, cache, rows=rows, max_len=LOOP_MAX_LEN, draft_len=K, ngram_max=NGRAM, sync_every=SYNC, graph=graph), cache


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_spec_loop_with_fuse_verify(dev, dtype, monkeypatch):
    from qqq_amd import ops
    from test_gpu_spec_loop import K, N_NEW, VOCAB, _blocks, _prompts, _reference

    lm = _lm(dev, 128, "verify")
    prompts = _prompts()[1:]  # two rows
    nb = sum(_blocks(prompts))
    calls = []
    for name in ("verify_attention_paged", "verify_attention_paged_kv8"):
        real = getattr(ops, name)
        monkeypatch.setattr(f"qqq_amd.attention.ops.{name}", lambda *a, _n=name, _f=real, **kw: (calls.append(_n), _f(*a, **kw))[1])
    with torch.no_grad():
        want, accepted, _ = _reference(lm, prompts, N_NEW, dtype, rows=2)
        print(f"accepted drafts per row-step with fuse_verify() ({dtype}): {accepted}")
        assert any(a > 0 for a in accepted) and any(a < K for a in accepted), accepted  # some drafts accepted, some refused
        assert calls and set(calls) == {"verify_attention_paged" + ("_kv8" if dtype == torch.int8 else "")}
        eager, c_e = _spec_loop(lm, dtype, False, nb, 2)
        got = eager.generate(prompts, N_NEW)
        assert got == want and all(len(o) == N_NEW and all(0 <= x < VOCAB for x in o) for o in got)
        assert eager.accepted == sum(accepted) and eager.row_steps == len(accepted)
        graph, c_g = _spec_loop(lm, dtype, True, nb, 2)
        assert graph.generate(prompts, N_NEW) == got
        assert (graph.accepted, graph.row_steps, graph.steps) == (eager.accepted, eager.row_steps, eager.steps)
    assert eager.captures == 0 and graph.captures == 1 and c_e.free_blocks == nb and c_g.free_blocks == nb


def test_idle_rows_are_inert_with_fuse_verify(dev):
    """tests/test_gpu_spec_loop.py::test_idle_rows_are_inert on the verify path: the idle row of a 3-row batch carries NaN from the embedding
    on; the two active rows' tokens do not change and nothing of it reaches the pool."""
    from test_gpu_spec_loop import G, LAYERS, N_NEW, VOCAB, _blocks, _prompts

    rows = 3
    lm = _lm(dev, 128, "verify")
    prompts = _prompts()[1:]
    nb = sum(_blocks(prompts))

    def poison(mod, inp, out):
        if out.shape[0] != rows * G:  # the packed prefill
            return None
        out = out.clone()
        out[(rows - 1) * G:] = float("nan")
        return out

    with torch.no_grad():
        for dtype in (torch.float16, torch.int8):
            clean, _ = _spec_loop(lm, dtype, False, nb, rows)
            want = clean.generate(prompts, N_NEW)
            hook = lm.model.embed_tokens.register_forward_hook(poison)
            try:
                for graph in (False, True):
                    loop, cache = _spec_loop(lm, dtype, graph, nb, rows)
                    loop.ids[rows - 1] = VOCAB - 1
                    assert loop.generate(prompts, N_NEW) == want, (dtype, graph)
                    assert loop.start[rows - 1].item() == -1 and loop.n_out[rows - 1].item() == 0
                    for l in range(LAYERS):
                        pools = (cache.k[l], cache.v[l]) + ((cache.k_scale[l], cache.v_scale[l]) if cache.quantized else ())
                        assert all(torch.isfinite(x.float()).all() for x in pools)
                    assert torch.isnan(lm(loop.ids.view(-1), cache, loop.step, all_rows=True)[(rows - 1) * G:]).any()
            finally:
                hook.remove()
