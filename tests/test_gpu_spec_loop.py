"""SpecDecodeLoop on the GPU: the eager loop against a reference loop written here from public pieces (a hand-built PagedStep of G-token
chunks with an idle row, lm(all_rows=True), ops.sample_tokens, tests/spec_ref.py), the captured loop against the eager one, idle rows that
carry NaN, continuous batching through a pool of two budgets, what "greedy" still means, and generate(device_loop=True, draft_len=K).

The model has a vocabulary of 8 and embeddings scaled up against the layers' updates, so that the next token depends mostly on the last
one and 1- and 2-gram drafts come true often enough: the reference loop's steps accept no draft, some and all of them (asserted)."""
import numpy as np
import pytest
import torch

import spec_ref
from test_gpu_attn import _make_layer
from test_gpu_model import HEADS, HIDDEN, INTER, KVH, LAYERS, PROMPT_LENS, _manual

pytestmark = pytest.mark.gpu

VOCAB, ROWS, MAX_LEN, BS, K, NGRAM, N_NEW, SYNC = 8, 4, 64, 16, 3, 3, 12, 3
G = K + 1
MODEL_SEED, PROMPT_SEED, EMBED_SCALE = 5, 3, 4.0  # chosen on an MI355X for the precondition of _check_acceptance
SAMPLED = dict(temperature=0.8, top_k=50, top_p=0.9)


def _make_lm(dev, gs, seed=MODEL_SEED, scale=EMBED_SCALE):
    from qqq_amd import QuantLlamaForCausalLM, QuantLlamaModel

    with torch.random.fork_rng(devices=[dev]):
        torch.manual_seed(seed)  # the layers' norm weights come from the default generator
        layers = [_make_layer(dev, HIDDEN, HEADS, KVH, INTER, gs, False, seed + 10 * i) for i in range(LAYERS)]
    for i, layer in enumerate(layers):
        layer.self_attn.layer_idx = i
    lm = QuantLlamaForCausalLM(QuantLlamaModel(VOCAB, LAYERS, HIDDEN, HEADS, KVH, INTER, gs, rms_norm_eps=1e-6, layers=layers)).to(dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    lm.model.embed_tokens.weight.data = (scale * torch.randn((VOCAB, HIDDEN), generator=g, device=dev)).half()
    lm.model.norm.weight.data = (1 + 0.1 * torch.randn(HIDDEN, generator=g, device=dev)).half()
    lm.lm_head.weight.data = (0.2 * torch.randn((VOCAB, HIDDEN), generator=g, device=dev)).half()
    return lm.eval().fuse_prefill()


def _prompts(seed=PROMPT_SEED, lens=PROMPT_LENS):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in lens]


def _blocks(prompts, n_new=N_NEW):
    return [-(-(len(p) + n_new - 1 + K) // BS) for p in prompts]


def _match_end(h, nmax):
    """the end position c of the occurrence the drafter continues from: the deepest n <= nmax, then the largest c <= L - 2; None: no match"""
    last = len(h) - 1
    for n in range(min(nmax, last), 0, -1):
        for c in range(last - 1, n - 2, -1):
            if all(h[c - t] == h[last - t] for t in range(n)):
                return c
    return None


def _reference(lm, prompts, n_new, dtype, eos=None, sample=None, seed=None, max_len=MAX_LEN, rows=ROWS, ends=None):
    """`prompts` in rows 0 ... of a `rows`-row batch, the other rows idle: the packed prefill, then per step a hand-built PagedStep of
    G-token chunks, lm(all_rows=True), ops.sample_tokens with the variates the loop documents, and spec_ref.advance on the host.
    -> (the tokens per prompt, the accepted drafts of every row-step, {(prompt, position): the logits row its token was drawn from});
    `ends`, a list, receives (prompt, c) for every draft that came from a match: where the scan found it"""
    from qqq_amd import PagedStep, ops

    dev = lm.lm_head.weight.device
    T, top_k, top_p = (sample["temperature"], sample["top_k"], sample["top_p"]) if sample else (0.0, 0, 1.0)
    gen = torch.Generator(device=dev).manual_seed(seed) if seed is not None else None
    cache = lm.new_cache(sum(_blocks(prompts, n_new)), BS, dtype)
    sids = list(range(len(prompts)))
    for s in sids:
        cache.add(s)
        cache.reserve(s, len(prompts[s]) + n_new - 1 + K)
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=dev)
    logits = lm(ids, cache, cache.step(sids, [len(p) for p in prompts]))
    first = ops.sample_tokens(logits, T, top_k, top_p, torch.rand(len(prompts), generator=gen, device=dev)).tolist()
    seen = {(s, len(prompts[s])): logits[s].clone() for s in sids}
    st = spec_ref.new_state(rows, K, -(-max_len // BS), max_len, BS)
    for s in sids:
        if n_new > 1 and first[s] != eos:
            spec_ref.seat(st, s, prompts[s] + [first[s]], cache.blocks(s), n_new - 1, NGRAM, -1 if eos is None else eos)
    u_stride = SYNC * G
    used, u, accepted = u_stride, None, []
    cu = torch.arange(rows + 1, dtype=torch.int32, device=dev) * G
    table = torch.from_numpy(st["block_table"]).to(dev)
    while (st["remaining"] > 0).any():
        steps = min(SYNC, int(st["remaining"].max()))  # the loop's window: what it read at its last sync
        if used + steps * G > u_stride:
            u = torch.rand((rows, u_stride), generator=gen, device=dev)
            st["tick"][:] = 0
            used = 0
        used += steps * G
        for _ in range(steps):
            start = torch.from_numpy(st["start"]).to(dev)
            step = PagedStep(seq_ids=[None] * rows, counts=[G] * rows, starts=[0] * rows, max_len=max_len, decode=False,
                             pos=torch.from_numpy(st["pos"]).to(dev).view(-1), slots=torch.from_numpy(st["slots"]).to(dev).view(-1),
                             block_table=table, last_pos=start, cu_tokens=cu, start_pos=start)
            logits = lm(torch.from_numpy(st["ids"]).to(dev).view(-1), cache, step, all_rows=True)
            idx = (torch.from_numpy(st["tick"]).to(dev).long()[:, None] * G + torch.arange(G, device=dev)[None]) % u_stride
            toks = ops.sample_tokens(logits, T, top_k, top_p, u.gather(1, idx).reshape(-1).contiguous()).view(rows, G).tolist()
            live = [r for r in range(rows) if st["remaining"][r] > 0]
            before = {r: (int(st["hist_len"][r]), int(st["n_acc"][r])) for r in live}
            spec_ref.advance(st, toks, NGRAM)
            for r in live:
                n0, a0 = before[r]
                accepted.append(int(st["n_acc"][r]) - a0)
                for j in range(int(st["hist_len"][r]) - n0):  # token n0 + j of the sequence was drawn from logits row r * G + j
                    seen[(r, n0 + j)] = logits[r * G + j].clone()
                if ends is not None and st["remaining"][r] > 0:
                    c = _match_end(st["hist"][r, :int(st["hist_len"][r])].tolist(), NGRAM)
                    if c is not None:
                        ends.append((r, c))
    outs = []
    for s in sids:
        n = int(st["hist_len"][s])
        outs.append([first[s]] + (st["hist"][s, len(prompts[s]) + 1:n].tolist() if n else []))
    return outs, accepted, seen


def _check_acceptance(accepted):
    """the precondition that keeps these tests from passing vacuously: the reference's row-steps accepted every draft, some, and none"""
    assert K in accepted and 0 in accepted and any(0 < a < K for a in accepted), accepted


def _loop(lm, dtype, graph, num_blocks, rows=ROWS, max_len=MAX_LEN):
    from qqq_amd import SpecDecodeLoop

    cache = lm.new_cache(num_blocks, BS, dtype)
    return SpecDecodeLoop(lm, cache, rows=rows, max_len=max_len, draft_len=K, ngram_max=NGRAM, sync_every=SYNC, graph=graph), cache


@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_eager_loop_equals_the_reference(dev, dtype, gs):
    lm = _make_lm(dev, gs)
    prompts = _prompts()
    nb = sum(_blocks(prompts))
    with torch.no_grad():
        want, accepted, _ = _reference(lm, prompts, N_NEW, dtype)
        print(f"accepted drafts per row-step ({dtype}, gs {gs}): {accepted}")
        _check_acceptance(accepted)
        eager, cache = _loop(lm, dtype, False, nb)
        got = eager.generate(prompts, N_NEW)
        assert got == want and all(len(o) == N_NEW and all(0 <= t < VOCAB for t in o) for o in got)
        assert eager.accepted == sum(accepted) and eager.row_steps == len(accepted) and eager.steps >= max(1, len(accepted) // 3)
        # an eos taken from that run: the sequence stops there, the others go on as before
        eos = want[1][2]
        stopped, _, _ = _reference(lm, prompts, N_NEW, dtype, eos=eos)
        assert stopped == [o[:o.index(eos) + 1] if eos in o else o for o in want] and len(stopped[1]) <= 3
        assert eager.generate(prompts, N_NEW, eos_token_id=eos) == stopped
        # sampled, under equally seeded generators
        sampled, _, _ = _reference(lm, prompts, N_NEW, dtype, sample=SAMPLED, seed=77)
        g = torch.Generator(device=dev).manual_seed(77)
        assert eager.generate(prompts, N_NEW, generator=g, **SAMPLED) == sampled and all(len(o) == N_NEW for o in sampled)
        assert sampled != want  # 36 draws at temperature 0.8 over 8 tokens
        assert eager.generate(prompts, 1) == [o[:1] for o in want]
    assert eager.captures == 0 and cache.free_blocks == nb


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_captured_loop_equals_the_eager_one(dev, dtype):
    lm = _make_lm(dev, 128)
    prompts = _prompts()
    nb = sum(_blocks(prompts))
    with torch.no_grad():
        eager, c_e = _loop(lm, dtype, False, nb)
        graph, c_g = _loop(lm, dtype, True, nb)
        got = eager.generate(prompts, N_NEW)
        assert graph.generate(prompts, N_NEW) == got
        assert (graph.accepted, graph.row_steps, graph.steps) == (eager.accepted, eager.row_steps, eager.steps)
        eos = got[1][2]
        assert graph.generate(prompts, N_NEW, eos_token_id=eos) == eager.generate(prompts, N_NEW, eos_token_id=eos)
        runs = []
        for loop in (eager, graph):
            g = torch.Generator(device=dev).manual_seed(77)
            runs.append(loop.generate(prompts, N_NEW, generator=g, **SAMPLED))
        assert runs[0] == runs[1] and runs[0] != got
        assert graph.generate(prompts, 1) == [o[:1] for o in got]
    assert eager.captures == 0 and graph.captures == 1
    assert c_e.free_blocks == nb and c_g.free_blocks == nb


LONG_MAX_LEN, LONG_NEW = 320, 24
# 290 tokens, a period of two per stretch: the latest occurrence of 1 ends at position 59 (wave 0 of the scan's first pass), of 2 and 3 at
# 120 and 121 (wave 1), of 4 and 5 at 182 and 183 (wave 2), of 0 at 244 (wave 3); the last stretch, the one the first drafts continue,
# ends beyond 256, on the second pass
LONG_PROMPT = [0, 1] * 30 + [2, 3] * 31 + [4, 5] * 31 + [0, 6] * 31 + [7, 6] * 22


def test_long_history_loops_equal_the_reference(dev):
    """the greedy comparison of the two tests above once more in a loop of max_len 320 with a prompt of 290 tokens beside the others: the
    drafter's scan takes a second pass, and the long row's matches end beyond position 256 as well as past wave 0 of the first pass
    (asserted on the reference's)"""
    lm = _make_lm(dev, 128)
    prompts = _prompts() + [LONG_PROMPT]
    assert len(LONG_PROMPT) == 290 and len(prompts) == ROWS
    nb = sum(_blocks(prompts, LONG_NEW))
    ends = []
    with torch.no_grad():
        want, accepted, _ = _reference(lm, prompts, LONG_NEW, torch.float16, max_len=LONG_MAX_LEN, rows=ROWS + 1, ends=ends)
        where = sorted({((c % 256) // 64, c // 256) for r, c in ends if r == ROWS - 1})
        print(f"accepted drafts per row-step: {accepted}; the long prompt's matches ended in (wave, pass) {where}: {ends}")
        _check_acceptance(accepted)
        assert any(p == 1 for _, p in where) and any(p == 0 and w >= 1 for w, p in where), where
        eager, c_e = _loop(lm, torch.float16, False, nb, rows=ROWS + 1, max_len=LONG_MAX_LEN)
        graph, c_g = _loop(lm, torch.float16, True, nb, rows=ROWS + 1, max_len=LONG_MAX_LEN)
        assert eager.generate(prompts, LONG_NEW) == want and all(len(o) == LONG_NEW for o in want)
        assert eager.accepted == sum(accepted) and eager.row_steps == len(accepted)
        assert graph.generate(prompts, LONG_NEW) == want
        assert (graph.accepted, graph.row_steps, graph.steps) == (eager.accepted, eager.row_steps, eager.steps)
    assert eager.captures == 0 and graph.captures == 1 and c_e.free_blocks == nb and c_g.free_blocks == nb


def test_idle_rows_are_inert(dev):
    """Row 3 of the 4-row batch is idle throughout.  Its embedding rows are set to NaN in every step of the loop, so its q rows, its
    activations and its logits are NaN from the first layer on: the three active rows' tokens do not change, and nothing of it reaches the
    pool."""
    lm = _make_lm(dev, 128)
    prompts = _prompts()
    nb = sum(_blocks(prompts))

    def poison(mod, inp, out):
        if out.shape[0] != ROWS * G:  # the packed prefill
            return None
        out = out.clone()
        out[(ROWS - 1) * G:] = float("nan")
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
                    assert loop.start[ROWS - 1].item() == -1 and loop.n_out[ROWS - 1].item() == 0 and loop.hist_len[ROWS - 1].item() == 0
                    assert loop.ids[ROWS - 1].tolist() == [VOCAB - 1] * G
                    for l in range(LAYERS):
                        pools = (cache.k[l], cache.v[l]) + ((cache.k_scale[l], cache.v_scale[l]) if cache.quantized else ())
                        assert all(torch.isfinite(t.float()).all() for t in pools)
                    # the hook did poison the row: the idle row's logits are NaN
                    assert torch.isnan(lm(loop.ids.view(-1), cache, loop.step, all_rows=True)[(ROWS - 1) * G:]).any()
            finally:
                hook.remove()


def test_continuous_batching_through_a_pool_of_two_budgets(dev):
    lm = _make_lm(dev, -1)
    prompts = _prompts(seed=11, lens=(5, 17, 33, 9, 21))
    assert _blocks(prompts) == [2, 2, 3, 2, 3]  # 19, 31, 47, 23 and 35 keys, the K drafts included
    with torch.no_grad():
        loop, cache = _loop(lm, torch.float16, True, 6, rows=2)  # the two largest budgets, and never three of the five
        got = loop.generate(prompts, N_NEW)
        assert all(len(o) == N_NEW for o in got) and cache.free_blocks == 6
        for p, o in zip(prompts, got):
            assert loop.generate([p], N_NEW) == [o]
        assert loop.captures == 1 and cache.free_blocks == 6
        eager, c_e = _loop(lm, torch.float16, False, 6, rows=2)
        assert eager.generate(prompts, N_NEW) == got and c_e.free_blocks == 6
        # the K keys of the drafts count: 5 + 12 - 1 = 16 keys are one block, 19 are two.  The pool that is one block short raises and
        # is left as it was found
        small, c_s = _loop(lm, torch.float16, False, 4, rows=2)
        c_s.add("other")
        c_s.reserve("other", 3 * BS)
        with pytest.raises(RuntimeError, match="cannot hold a prompt"):
            small.generate(prompts[:1], N_NEW)
        assert c_s.free_blocks == 1 and (small.remaining == 0).all() and (small.start == -1).all()
        c_s.free("other")
        assert small.generate(prompts[:1], N_NEW) == got[:1] and c_s.free_blocks == 4


def _teacher_forced(lm, prompts, outs, seen):
    """prompt + output through one fused-prefill chunk, every row's logits -> (D, {(prompt, position): the f32 logits row that predicts
    that position}); D is the largest absolute difference to the logits rows `seen` (the reference loop's) at the same positions"""
    dev = lm.lm_head.weight.device
    full = [p + o for p, o in zip(prompts, outs)]
    cache = lm.new_cache(sum(-(-len(f) // BS) for f in full), BS)
    for s in range(len(full)):
        cache.add(s)
    ids = torch.tensor([t for f in full for t in f], dtype=torch.int64, device=dev)
    forced = lm(ids, cache, cache.step(list(range(len(full))), [len(f) for f in full]), all_rows=True).float()
    offs = np.cumsum([0] + [len(f) for f in full])
    rows = {(s, q): forced[offs[s] + q - 1] for s in range(len(full)) for q in range(len(prompts[s]), len(full[s]))}  # row q - 1 predicts q
    assert set(rows) == set(seen)
    return max(float((seen[key].float() - rows[key]).abs().max()) for key in rows), rows


def test_greedy_keeps_its_meaning(dev):
    """Teacher-force prompt + output through one fused-prefill chunk with every row's logits.  Every emitted token's logit must be within
    2 D of its row's maximum, D being the largest absolute difference between the logits the REFERENCE loop drew the tokens from and the
    teacher-forced logits of the same positions -- both may move by D; it stems from the fp16 lm_head GEMM at another row count alone.
    Positions whose teacher-forced top-two margin is within 2 D (where the argmax may legitimately differ) are at most one in eight."""
    lm = _make_lm(dev, 128)
    prompts = _prompts()
    nb = sum(_blocks(prompts))
    with torch.no_grad():
        want, accepted, seen = _reference(lm, prompts, N_NEW, torch.float16)
        _check_acceptance(accepted)
        loop, _ = _loop(lm, torch.float16, True, nb)
        got = loop.generate(prompts, N_NEW)
        d, rows = _teacher_forced(lm, prompts, want, seen)
    close = 0
    for s, out in enumerate(got):
        assert len(out) == N_NEW
        # teacher forcing followed the reference's tokens: a loop that left them is judged up to where it did
        for j, t in enumerate(out):
            row = rows[(s, len(prompts[s]) + j)]
            top = torch.sort(row, descending=True).values
            print(f"prompt {s} token {j}: logit {float(row[t]):.4f} max {float(top[0]):.4f} margin {float(top[0] - top[1]):.4f} D {d:.4g}")
            assert float(top[0] - row[t]) <= 2 * d, (s, j, t, float(top[0] - row[t]), d)
            close += float(top[0] - top[1]) <= 2 * d
            if t != want[s][j]:
                break
    assert close * 8 <= len(prompts) * N_NEW, (close, d)


def test_generate_draft_len_is_the_spec_loop_and_the_other_paths_are_unchanged(dev):
    from qqq_amd import DecodeLoop, SpecDecodeLoop

    lm = _make_lm(dev, 128)
    prompts = _prompts()
    need = _blocks(prompts)
    with torch.no_grad():
        cache = lm.new_cache(sum(need), BS)
        want = SpecDecodeLoop(lm, cache, rows=len(prompts), max_len=max(need) * BS, draft_len=K).generate(prompts, N_NEW)
        assert lm.generate(prompts, N_NEW, device_loop=True, draft_len=K) == want
        assert lm.generate(prompts, N_NEW, device_loop=True, draft_len=K, cache=cache) == want and cache.free_blocks == sum(need)
        g1, g2 = (torch.Generator(device=dev).manual_seed(5) for _ in range(2))
        sampled = lm.generate(prompts, N_NEW, generator=g1, device_loop=True, draft_len=K, **SAMPLED)
        assert sampled == SpecDecodeLoop(lm, cache, rows=len(prompts), max_len=max(need) * BS, draft_len=K).generate(
            prompts, N_NEW, generator=g2, **SAMPLED)
        # the paths without drafts: what tests/test_gpu_model.py and tests/test_gpu_decode_loop.py hold them to
        plain = [-(-(len(p) + N_NEW - 1) // BS) for p in prompts]
        assert lm.generate(prompts, N_NEW) == _manual(lm, prompts, N_NEW, 0.0, 0, 1.0, 0)
        assert lm.generate(prompts, N_NEW, device_loop=True) == DecodeLoop(lm, lm.new_cache(sum(plain), BS), rows=len(prompts),
                                                                           max_len=max(plain) * BS).generate(prompts, N_NEW)
        with pytest.raises(ValueError, match="device_loop=True"):
            lm.generate(prompts, N_NEW, draft_len=K)
