"""generate(logprobs=k) on the GPU, host path and DecodeLoop: the tokens are those of the same call without logprobs, and every record
equals ops.token_logprobs / ops.topk_logprobs of the logits row its token was drawn from, bit for bit -- the rows are captured by
wrappers around ops.sample_tokens and ops.sample_advance that keep a clone of each pass's logits.  The captured loop equals the eager one."""
import pytest
import torch

from test_gpu_model import VOCAB, _make_lm, _prompts

pytestmark = pytest.mark.gpu

K, N_NEW, ROWS, MAX_LEN, BS = 5, 6, 3, 48, 16
SAMPLED = dict(temperature=0.8, top_k=20, top_p=0.9)
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.2)


def _i32(t):
    return t.contiguous().view(torch.int32)


def _row_records(logits, toks):
    """the two ops on a captured pass: (logprob, rank, top_ids, top_logprobs) on the CPU, logprob held against the scoring kernel"""
    from qqq_amd import ops

    full = ops.topk_logprobs(logits, toks, K)
    scored, argmax = ops.token_logprobs(logits, toks)
    assert torch.equal(_i32(full[0]), _i32(scored)) and torch.equal(full[2][:, 0].long(), argmax)
    for i in range(K):
        again, _ = ops.token_logprobs(logits, full[2][:, i].long())
        assert torch.equal(_i32(full[3][:, i]), _i32(again))
    return [t.cpu() for t in full]


def _same_records(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        if isinstance(a, list):
            _same_records(a, b)
            continue
        assert all(x.device.type == "cpu" for x in a)
        assert a.logprob.shape == b[0].shape and a.top_ids.shape == b[2].shape == (a.logprob.shape[0], K)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and torch.equal(_i32(x), _i32(y))


# ---- the host path

@pytest.mark.parametrize("what", ["greedy", "sampled", "penalised", "n3"])
def test_host_path_records_are_the_ops_on_the_rows_the_sampler_drew_from(dev, monkeypatch, what):
    from qqq_amd import TokenLogprobs, ops

    lm = _make_lm(dev, 128).fuse_prefill()
    prompts = _prompts()
    kw = dict(greedy={}, sampled=SAMPLED, penalised=dict(SAMPLED, **PEN), n3=dict(SAMPLED, n=3))[what]
    n = kw.get("n", 1)
    with torch.no_grad():
        greedy = lm.generate(prompts, N_NEW)
        eos = greedy[1][2] if what == "greedy" else None  # ends a sequence early
        plain = lm.generate(prompts, N_NEW, generator=torch.Generator(device=dev).manual_seed(11), eos_token_id=eos, **kw)
        passes, real = [], ops.sample_tokens

        def sample_tokens(logits, *a):
            toks = real(logits, *a)
            passes.append((logits.clone(), toks.clone()))
            return toks

        with monkeypatch.context() as mp:
            mp.setattr(ops, "sample_tokens", sample_tokens)
            toks, recs = lm.generate(prompts, N_NEW, generator=torch.Generator(device=dev).manual_seed(11), eos_token_id=eos, logprobs=K, **kw)
        assert toks == plain and (what != "greedy" or len(toks[1]) <= 3)
        # one admission wave (the default pool holds everything): a pass's rows are the running completions in order
        flat_toks = [c for p in toks for c in p] if n > 1 else toks
        want = [[] for _ in flat_toks]
        running = list(range(len(flat_toks)))
        for logits, drawn in passes:
            assert logits.shape[0] == len(running)
            parts = _row_records(logits, drawn)
            for row, i in enumerate(running):
                assert flat_toks[i][len(want[i])] == int(drawn[row])
                want[i].append([p[row] for p in parts])
            running = [i for i in running if len(want[i]) < len(flat_toks[i])]
        assert not running
        want = [tuple(torch.stack([rec[j] for rec in seq]) for j in range(4)) for seq in want]
        flat_recs = [c for p in recs for c in p] if n > 1 else recs
        assert all(isinstance(r, TokenLogprobs) for r in flat_recs) and (n == 1 or [len(r) for r in recs] == [3] * len(prompts))
        _same_records(flat_recs, want)
        assert what != "greedy" or all(r.rank.tolist() == [1] * len(t) for r, t in zip(flat_recs, flat_toks))
        assert all((r.top_logprobs[:, :-1] >= r.top_logprobs[:, 1:]).all() and (r.logprob <= 0).all() for r in flat_recs)


# ---- the device loop

@pytest.mark.parametrize("what", ["greedy", "sampled"])
def test_decode_loop_records_and_captured_equals_eager(dev, monkeypatch, what):
    from qqq_amd import DecodeLoop, ops

    lm = _make_lm(dev, 128).fuse_prefill()
    prompts = _prompts() + [_prompts(seed=4)[0]]  # four prompts on three rows: rows are reused, and two are idle in the second wave
    nb = sum(-(-(len(p) + N_NEW - 1) // BS) for p in prompts)
    kw = {} if what == "greedy" else SAMPLED

    def gen():
        return torch.Generator(device=dev).manual_seed(23)

    with torch.no_grad():
        base = DecodeLoop(lm, lm.new_cache(nb, BS), rows=ROWS, max_len=MAX_LEN, sync_every=3, graph=False)
        free = base.generate(prompts, N_NEW, generator=gen(), **kw)
        eos = free[1][2]  # ends sequence 1 after three tokens
        plain = base.generate(prompts, N_NEW, generator=gen(), eos_token_id=eos, **kw)
        assert len(plain[1]) <= 3
        eager = DecodeLoop(lm, lm.new_cache(nb, BS), rows=ROWS, max_len=MAX_LEN, sync_every=3, graph=False, logprobs=K)
        firsts, sessions, real_first, real_step = [], [[] for _ in range(ROWS)], ops.sample_tokens, ops.sample_advance

        def sample_tokens(logits, *a):
            toks = real_first(logits, *a)
            firsts.append((logits.clone(), toks.clone()))
            return toks

        def sample_advance(logits, *a):
            out, n_out = a[11], a[12]
            before = n_out.clone()
            real_step(logits, *a)
            emitted = (n_out > before).nonzero()[:, 0].tolist()
            assert (n_out - before).max() <= 1
            if emitted:
                at = torch.tensor(emitted, device=dev)
                drawn = out[at, before[at].long()]
                parts = _row_records(logits[at], drawn)
                for j, r in enumerate(emitted):
                    if int(before[r]) == 0:
                        sessions[r].append([])  # the row serves a new sequence
                    sessions[r][-1].append((int(drawn[j]), [p[j] for p in parts]))

        with monkeypatch.context() as mp:
            mp.setattr(ops, "sample_tokens", sample_tokens)
            mp.setattr(ops, "sample_advance", sample_advance)
            toks, recs = eager.generate(prompts, N_NEW, generator=gen(), eos_token_id=eos, **kw)
        assert toks == plain
        # the first records: the admission passes' rows are the prompts in order
        first = [torch.cat([_row_records(l, t)[j] for l, t in firsts]) for j in range(4)]
        assert first[0].shape[0] == len(prompts)
        # the others: a row's sessions, matched to the completions by the tokens they emitted
        tails = {tuple(t[1:]): i for i, t in enumerate(toks) if len(t) > 1}
        assert len(tails) == sum(len(t) > 1 for t in toks)  # no two completions share their tail
        found = {}
        for r in range(ROWS):
            for session in sessions[r]:
                found[tails[tuple(t for t, _ in session)]] = session
        assert sorted(found) == sorted(tails.values())
        want = []
        for i in range(len(prompts)):
            rows = [[p[i] for p in first]] + [rec for _, rec in found.get(i, [])]
            want.append(tuple(torch.stack([rec[j] for rec in rows]) for j in range(4)))
        _same_records(recs, want)
        assert [r.logprob.shape[0] for r in recs] == [len(t) for t in toks]
        assert eager.n_rec.tolist() == eager.n_out.tolist()
        # the captured loop: the same tokens and the same bits
        graph = DecodeLoop(lm, lm.new_cache(nb, BS), rows=ROWS, max_len=MAX_LEN, sync_every=3, graph=True, logprobs=K)
        for _ in range(2):  # ... again when the loop is reused
            g_toks, g_recs = graph.generate(prompts, N_NEW, generator=gen(), eos_token_id=eos, **kw)
            assert g_toks == toks
            _same_records(g_recs, [tuple(r) for r in recs])
        assert graph.captures == 1 and eager.captures == 0 and graph.cache.free_blocks == nb and eager.cache.free_blocks == nb
        assert all(0 <= t < VOCAB for r in g_recs for t in r.top_ids.flatten().tolist())
