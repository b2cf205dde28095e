"""Repetition, presence and frequency penalties through the three generate paths on the GPU: DecodeLoop and SpecDecodeLoop built with
penalties=True against reference loops written here from public pieces (a hand-built PagedStep, tests/penalty_ref.py on the logits,
ops.sample_tokens, host bookkeeping), the captured loops against the eager ones, lm.generate's three paths against each other, a
property that needs no reference (a large presence penalty: no token twice), idle rows that carry NaN, and a loop reused without
penalties.  The models and prompts are those of tests/test_gpu_model.py (DecodeLoop) and tests/test_gpu_spec_loop.py (the speculative
loop and the three paths: a vocabulary of 8, where drafts come true and tokens repeat)."""
import numpy as np
import pytest
import torch

import penalty_ref
import spec_ref
from test_gpu_decode_loop import _blocks as _plain_blocks
from test_gpu_model import LAYERS, VOCAB, _make_lm, _prompts
from test_gpu_spec_loop import G, K, NGRAM, SYNC
from test_gpu_spec_loop import VOCAB as SPEC_VOCAB
from test_gpu_spec_loop import _blocks as _spec_blocks
from test_gpu_spec_loop import _make_lm as _make_spec_lm
from test_gpu_spec_loop import _prompts as _spec_prompts

pytestmark = pytest.mark.gpu

ROWS, MAX_LEN, BS, N_NEW, SPEC_NEW = 4, 64, 16, 8, 12
PV = (1.3, 0.5, 0.25)
PEN = dict(repetition_penalty=PV[0], presence_penalty=PV[1], frequency_penalty=PV[2])
SAMPLED = dict(temperature=0.8, top_k=50, top_p=0.9)


def _penalised(logits, ids, pos, seen, n_prompt):
    """tests/penalty_ref.py on device logits -> (the penalised logits on the device, seen with the rows' input tokens recorded)"""
    got, seen = penalty_ref.penalize(logits.cpu().numpy(), np.asarray(ids, np.int64), np.asarray(pos, np.int64), seen,
                                     np.asarray(n_prompt, np.int32), *PV)
    return torch.from_numpy(got).to(logits.device), seen


def _prefill(lm, prompts, cache, sids):
    """the packed prefill and each prompt's first token, drawn from the logits penalised over the prompt (every index a prompt index)"""
    from qqq_amd import ops

    dev = lm.lm_head.weight.device
    ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=dev)
    logits = lm(ids, cache, cache.step(sids, [len(p) for p in prompts]))
    lens = [len(p) for p in prompts]
    seen = np.array([p + [-1] * (max(lens) - len(p)) for p in prompts], np.int32)
    logits, _ = _penalised(logits, [p[-1] for p in prompts], [n - 1 for n in lens], seen, lens)
    return logits, ops.sample_tokens(logits, 0.0, 0, 1.0, torch.zeros(len(prompts), device=dev)).tolist()


def _reference(lm, prompts, n_new, dtype, rows=ROWS):
    """test_gpu_decode_loop._reference with the penalties: greedy decoding of `prompts` in rows 0 ... of a `rows`-row batch at max_len =
    MAX_LEN, the other rows idle at pos -1; per token lm(ids, cache, PagedStep(...)), penalty_ref over the row's prompt and outputs,
    ops.sample_tokens, and the bookkeeping on the host."""
    from qqq_amd import PagedStep, ops

    dev = lm.lm_head.weight.device
    cache = lm.new_cache(sum(_plain_blocks(prompts, n_new)), BS, dtype)
    sids = list(range(len(prompts)))
    for s in sids:
        cache.add(s)
        cache.reserve(s, len(prompts[s]) + n_new - 1)
    _, first = _prefill(lm, prompts, cache, sids)
    outs = [[t] for t in first]
    table = torch.zeros((rows, -(-MAX_LEN // BS)), dtype=torch.int32)
    seen, n_prompt = np.zeros((rows, MAX_LEN), np.int32), np.zeros(rows, np.int32)
    cur, pos = [0] * rows, [-1] * rows
    for s in sids:
        table[s, :len(cache.blocks(s))] = torch.tensor(cache.blocks(s), dtype=torch.int32)
        seen[s, :len(prompts[s])], n_prompt[s] = prompts[s], len(prompts[s])
        if n_new > 1:
            cur[s], pos[s] = first[s], len(prompts[s])
    table_dev, zero = table.to(dev), torch.zeros(rows, device=dev)
    cu = torch.arange(rows + 1, dtype=torch.int32, device=dev)
    while any(p >= 0 for p in pos):
        slots = [-1 if p < 0 else int(table[r, p // BS]) * BS + p % BS for r, p in enumerate(pos)]
        pos_dev = torch.tensor(pos, dtype=torch.int64, device=dev)
        step = PagedStep(seq_ids=[None] * rows, counts=[1] * rows, starts=[0] * rows, max_len=MAX_LEN, decode=True, pos=pos_dev,
                         slots=torch.tensor(slots, dtype=torch.int64, device=dev), block_table=table_dev, last_pos=pos_dev, cu_tokens=cu,
                         start_pos=pos_dev)
        logits = lm(torch.tensor(cur, dtype=torch.int64, device=dev), cache, step)
        logits, seen = _penalised(logits, cur, pos, seen, n_prompt)
        toks = ops.sample_tokens(logits, 0.0, 0, 1.0, zero).tolist()
        for r in range(rows):
            if pos[r] < 0:
                continue
            outs[r].append(toks[r])
            cur[r], pos[r] = (0, -1) if len(outs[r]) >= n_new else (toks[r], pos[r] + 1)
    return outs


def _spec_reference(lm, prompts, n_new, dtype, rows=ROWS):
    """test_gpu_spec_loop._reference, greedy, with the penalties: the same chunks of G tokens per row; logits row j of a row is penalised
    over the row's history and its drafts 1 ... j before ops.sample_tokens draws from it.
    -> (the tokens per prompt, the accepted drafts of every row-step, {(prompt, position): the PENALISED logits row its token came from})"""
    from qqq_amd import PagedStep, ops

    dev = lm.lm_head.weight.device
    cache = lm.new_cache(sum(_spec_blocks(prompts, n_new)), BS, dtype)
    sids = list(range(len(prompts)))
    for s in sids:
        cache.add(s)
        cache.reserve(s, len(prompts[s]) + n_new - 1 + K)
    logits, first = _prefill(lm, prompts, cache, sids)
    drawn = {(s, len(prompts[s])): logits[s].clone() for s in sids}
    st = spec_ref.new_state(rows, K, -(-MAX_LEN // BS), MAX_LEN, BS)
    n_prompt = np.zeros(rows, np.int32)
    for s in sids:
        n_prompt[s] = len(prompts[s])
        if n_new > 1:
            spec_ref.seat(st, s, prompts[s] + [first[s]], cache.blocks(s), n_new - 1, NGRAM, -1)
    accepted = []
    cu = torch.arange(rows + 1, dtype=torch.int32, device=dev) * G
    table, zero = torch.from_numpy(st["block_table"]).to(dev), torch.zeros(rows * G, device=dev)
    while (st["remaining"] > 0).any():
        start = torch.from_numpy(st["start"]).to(dev)
        step = PagedStep(seq_ids=[None] * rows, counts=[G] * rows, starts=[0] * rows, max_len=MAX_LEN, decode=False,
                         pos=torch.from_numpy(st["pos"]).to(dev).view(-1), slots=torch.from_numpy(st["slots"]).to(dev).view(-1),
                         block_table=table, last_pos=start, cu_tokens=cu, start_pos=start)
        logits = lm(torch.from_numpy(st["ids"]).to(dev).view(-1), cache, step, all_rows=True)
        logits, hist = _penalised(logits, st["ids"], st["pos"], st["hist"], n_prompt)
        assert np.array_equal(hist, st["hist"])  # the op's write into the loop's history is the identity
        toks = ops.sample_tokens(logits, 0.0, 0, 1.0, zero).view(rows, G).tolist()
        live = [r for r in range(rows) if st["remaining"][r] > 0]
        before = {r: (int(st["hist_len"][r]), int(st["n_acc"][r])) for r in live}
        spec_ref.advance(st, toks, NGRAM)
        for r in live:
            n0, a0 = before[r]
            accepted.append(int(st["n_acc"][r]) - a0)
            for j in range(int(st["hist_len"][r]) - n0):
                drawn[(r, n0 + j)] = logits[r * G + j].clone()
    outs = [[first[s]] + st["hist"][s, len(prompts[s]) + 1:int(st["hist_len"][s])].tolist() for s in sids]
    return outs, accepted, drawn


def _loops(lm, dtype, nb, spec, **kw):
    from qqq_amd import DecodeLoop, SpecDecodeLoop

    made = []
    for graph in (False, True):
        cache = lm.new_cache(nb, BS, dtype)
        if spec:
            made.append(SpecDecodeLoop(lm, cache, rows=ROWS, max_len=MAX_LEN, draft_len=K, ngram_max=NGRAM, sync_every=SYNC, graph=graph, **kw))
        else:
            made.append(DecodeLoop(lm, cache, rows=ROWS, max_len=MAX_LEN, sync_every=3, graph=graph, **kw))
    return made


@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_decode_loop_equals_the_reference_and_captured_equals_eager(dev, dtype, gs):
    lm = _make_lm(dev, gs).fuse_prefill()
    prompts = _prompts()
    nb = sum(_plain_blocks(prompts))
    with torch.no_grad():
        want = _reference(lm, prompts, N_NEW, dtype)
        eager, graph = _loops(lm, dtype, nb, False, penalties=True)
        got = eager.generate(prompts, N_NEW, **PEN)
        plain = eager.generate(prompts, N_NEW)
        print(f"penalised {got}\nplain     {plain}")
        assert got == want and all(len(o) == N_NEW and all(0 <= t < VOCAB for t in o) for o in got)
        assert graph.generate(prompts, N_NEW, **PEN) == got
        runs = []
        for loop in (eager, graph):
            g = torch.Generator(device=dev).manual_seed(77)
            runs.append(loop.generate(prompts, N_NEW, generator=g, **SAMPLED, **PEN))
        assert runs[0] == runs[1] and runs[0] != got and all(len(o) == N_NEW for o in runs[0])
        assert graph.generate(prompts, 1, **PEN) == eager.generate(prompts, 1, **PEN) == [o[:1] for o in want]
    assert eager.captures == 0 and graph.captures == 1
    assert eager.cache.free_blocks == nb and graph.cache.free_blocks == nb
    assert int(torch.count_nonzero(eager.penalty_workspace)) == 0 and int(torch.count_nonzero(graph.penalty_workspace)) == 0


@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_spec_loop_equals_the_reference_and_captured_equals_eager(dev, dtype, gs):
    lm = _make_spec_lm(dev, gs)
    prompts = _spec_prompts()
    nb = sum(_spec_blocks(prompts, SPEC_NEW))
    with torch.no_grad():
        want, accepted, _ = _spec_reference(lm, prompts, SPEC_NEW, dtype)
        print(f"accepted drafts per row-step ({dtype}, gs {gs}): {accepted}\npenalised {want}")
        assert any(a > 0 for a in accepted), accepted  # a logits row behind an accepted draft was penalised over history + drafts
        eager, graph = _loops(lm, dtype, nb, True, penalties=True)
        assert eager.seen is eager.hist
        got = eager.generate(prompts, SPEC_NEW, **PEN)
        assert got == want and all(len(o) == SPEC_NEW and all(0 <= t < SPEC_VOCAB for t in o) for o in got)
        assert eager.accepted == sum(accepted) and eager.row_steps == len(accepted)
        assert graph.generate(prompts, SPEC_NEW, **PEN) == got
        assert (graph.accepted, graph.row_steps, graph.steps) == (eager.accepted, eager.row_steps, eager.steps)
        runs = []
        for loop in (eager, graph):
            g = torch.Generator(device=dev).manual_seed(77)
            runs.append(loop.generate(prompts, SPEC_NEW, generator=g, **SAMPLED, **PEN))
        assert runs[0] == runs[1] and runs[0] != got
    assert eager.captures == 0 and graph.captures == 1
    assert eager.cache.free_blocks == nb and graph.cache.free_blocks == nb
    assert int(torch.count_nonzero(eager.penalty_workspace)) == 0 and int(torch.count_nonzero(graph.penalty_workspace)) == 0


def _teacher_forced(lm, prompts, outs, drawn):
    """test_gpu_spec_loop._teacher_forced with both sides penalised: prompt + output through one fused-prefill chunk, the row that predicts
    position q penalised over the sequence in front of q -> (D, {(prompt, position): that f32 row}); D is the largest absolute difference
    to the penalised rows `drawn` (the reference loop's) at the same positions"""
    dev = lm.lm_head.weight.device
    full = [p + o for p, o in zip(prompts, outs)]
    cache = lm.new_cache(sum(-(-len(f) // BS) for f in full), BS)
    for s in range(len(full)):
        cache.add(s)
    ids = torch.tensor([t for f in full for t in f], dtype=torch.int64, device=dev)
    forced = lm(ids, cache, cache.step(list(range(len(full))), [len(f) for f in full]), all_rows=True)
    offs = np.cumsum([0] + [len(f) for f in full])
    keys = [(s, q) for s in range(len(full)) for q in range(len(prompts[s]), len(full[s]))]  # row q - 1 predicts position q
    assert set(keys) == set(drawn)
    width = max(len(f) for f in full)
    seen = np.array([full[s][:q - 1] + [-1] * (width - q + 1) for s, q in keys], np.int32)
    rows = forced[torch.tensor([int(offs[s]) + q - 1 for s, q in keys], device=dev)].contiguous()
    rows, _ = _penalised(rows, [full[s][q - 1] for s, q in keys], [q - 1 for s, q in keys], seen, [len(prompts[s]) for s, q in keys])
    rows = {key: rows[i].float() for i, key in enumerate(keys)}
    return max(float((drawn[key].float() - rows[key]).abs().max()) for key in keys), rows


def test_the_three_generate_paths_agree(dev):
    """lm.generate's host loop, device_loop=True and device_loop=True with draft_len=K under the same penalties, greedy, rows =
    len(prompts) and no eos (every path's head GEMM runs at comparable shapes).  The first two are equal.  The speculative path is judged
    as test_gpu_spec_loop.test_greedy_keeps_its_meaning judges it, on penalised logits: every emitted token's penalised logit within 2 D
    of its row's maximum, D the largest difference between the penalised logits the reference loop drew from and the teacher-forced ones;
    positions whose top-two margin is within 2 D are at most one in eight (asserted: the cap holds for these prompts)."""
    lm = _make_spec_lm(dev, 128).fuse_verify()
    prompts = _spec_prompts()
    with torch.no_grad():
        host = lm.generate(prompts, SPEC_NEW, **PEN)
        looped = lm.generate(prompts, SPEC_NEW, device_loop=True, **PEN)
        spec = lm.generate(prompts, SPEC_NEW, device_loop=True, draft_len=K, **PEN)
        print(f"host {host}\nloop {looped}\nspec {spec}")
        assert host == looped and all(len(o) == SPEC_NEW for o in host)
        want, accepted, drawn = _spec_reference(lm, prompts, SPEC_NEW, torch.float16, rows=len(prompts))
        d, rows = _teacher_forced(lm, prompts, want, drawn)
    close = 0
    for s, out in enumerate(spec):
        assert len(out) == SPEC_NEW
        for j, t in enumerate(out):  # teacher forcing followed the reference's tokens: a path that left them is judged up to where it did
            row = rows[(s, len(prompts[s]) + j)]
            top = torch.sort(row, descending=True).values
            print(f"prompt {s} token {j}: logit {float(row[t]):.4f} max {float(top[0]):.4f} margin {float(top[0] - top[1]):.4f} D {d:.4g}")
            assert float(top[0] - row[t]) <= 2 * d, (s, j, t, float(top[0] - row[t]), d)
            close += float(top[0] - top[1]) <= 2 * d
            if t != want[s][j]:
                break
    assert close * 8 <= len(prompts) * SPEC_NEW, (close, d)


def test_a_large_presence_penalty_never_repeats_a_token(dev):
    """presence_penalty = 3e4 puts every emitted token below every other one: the 7 < 8 generated tokens of every sequence are pairwise
    distinct on all three paths, whatever the logits.  The unpenalised greedy run of the same prompts does repeat tokens (asserted)."""
    lm = _make_spec_lm(dev, 128).fuse_verify()
    prompts = _spec_prompts()
    n_new = SPEC_VOCAB - 1
    with torch.no_grad():
        plain = lm.generate(prompts, n_new)
        assert all(len(set(o)) < len(o) for o in plain), plain
        for kw in ({}, dict(device_loop=True), dict(device_loop=True, draft_len=K)):
            outs = lm.generate(prompts, n_new, presence_penalty=3e4, **kw)
            print(kw, outs)
            assert all(len(o) == n_new and len(set(o)) == n_new for o in outs), (kw, outs)


@pytest.mark.parametrize("spec", [False, True])
def test_idle_rows_are_inert_and_a_loop_reused_without_penalties_is_the_plain_loop(dev, spec):
    """Row 3 of the 4-row batch is idle throughout; its embedding rows are NaN in every step, so its logits are NaN: the penalised tokens
    of the three active rows do not change, nothing of the row is recorded, and the workspace stays zero.  The same loops then serve a
    call with neutral values: the tokens of a loop built without the flag."""
    lm = _make_spec_lm(dev, 128) if spec else _make_lm(dev, 128).fuse_prefill()
    prompts = _spec_prompts() if spec else _prompts()
    n_new = SPEC_NEW if spec else N_NEW
    nb = sum(_spec_blocks(prompts, n_new) if spec else _plain_blocks(prompts, n_new))
    group = G if spec else 1

    def poison(mod, inp, out):
        if out.shape[0] != ROWS * group:  # the packed prefill
            return None
        out = out.clone()
        out[(ROWS - 1) * group:] = float("nan")
        return out

    with torch.no_grad():
        clean, _ = _loops(lm, torch.float16, nb, spec, penalties=True)
        want = clean.generate(prompts, n_new, **PEN)
        without, _ = _loops(lm, torch.float16, nb, spec)
        neutral = without.generate(prompts, n_new)
        hook = lm.model.embed_tokens.register_forward_hook(poison)
        try:
            for loop in _loops(lm, torch.float16, nb, spec, penalties=True):
                loop.seen[ROWS - 1] = 5
                assert loop.generate(prompts, n_new, **PEN) == want, loop.graph
                assert (loop.seen[ROWS - 1] == 5).all() and loop.pos[ROWS - 1].max().item() == -1 and loop.n_out[ROWS - 1].item() == 0
                assert int(torch.count_nonzero(loop.penalty_workspace)) == 0
                assert loop.repetition[:3].tolist() == [np.float32(PV[0])] * 3 and loop.repetition[3].item() == 1.0
                assert loop.generate(prompts, n_new) == neutral, loop.graph  # reused with neutral values
                assert loop.repetition.tolist() == [1.0] * ROWS and loop.presence.tolist() == [0.0] * ROWS
                assert loop.captures == int(loop.graph)
        finally:
            hook.remove()
    for layer in range(LAYERS):
        assert torch.isfinite(loop.cache.k[layer].float()).all()
