"""generate_guided on the GPU, greedy unless said otherwise, on the model and prompts of tests/test_gpu_model.py: the host path against the
free run of generate() (an automaton that allows everything changes nothing, a trie of choices is followed, a forbidden token yields the
free run's second most probable one), and GuidedDecodeLoop -- eager and captured, four prompts through three rows, several automata
through one capture -- against the host path."""
import pytest
import torch

from test_gpu_model import VOCAB, _make_lm, _prompts

pytestmark = pytest.mark.gpu

N_NEW, BS, ROWS, MAX_LEN = 12, 16, 3, 64


@pytest.fixture(scope="module")
def lm(dev):
    return _make_lm(dev, 128).fuse_prefill()


@pytest.fixture(scope="module")
def prompts():
    p = _prompts()
    return p + [p[1][::-1][:9]]  # a fourth: one more than the loops have rows


@pytest.fixture(scope="module")
def free(lm, prompts):
    """the free greedy run of the unchanged generate(), with its logprobs=2 records; never changed"""
    with torch.no_grad():
        out, recs = lm.generate(prompts, N_NEW, logprobs=2)
        assert lm.generate(prompts, N_NEW) == out
    assert all(len(o) == N_NEW for o in out)
    return out, recs


def _choices(free_out):
    """per prompt: the free run's first six tokens, and a decoy that shares two tokens with it and then differs"""
    from qqq_amd import TokenFSM

    return [TokenFSM.from_choices([c[:6], c[:2] + [(c[2] + 1) % VOCAB, 1, 2, 3]], vocab=VOCAB) for c in free_out]


def _without(free_out):
    """an automaton that follows free[0] for three tokens, forbids free[0][3] there, and allows everything from then on"""
    from qqq_amd import TokenFSM

    c = free_out[0]
    rest = [t for t in range(VOCAB) if t != c[3]]
    offsets = [0, 1, 2, 3, 3 + len(rest), 3 + len(rest) + VOCAB]
    return TokenFSM(offsets, c[:3] + rest + list(range(VOCAB)), [1, 2, 3] + [4] * len(rest) + [4] * VOCAB, [0, 0, 0, 0, 1], 0, VOCAB)


def _loop(lm, graph, **kw):
    from qqq_amd import GuidedDecodeLoop

    cache = lm.new_cache(ROWS * (MAX_LEN // BS), BS)
    return GuidedDecodeLoop(lm, cache, rows=ROWS, max_len=MAX_LEN, fsm_states=64, fsm_edges=4096, sync_every=3, graph=graph, **kw), cache


def test_the_host_path_follows_its_automata(lm, prompts, free):
    from qqq_amd import TokenFSM

    free_out, free_recs = free
    eos = next(t for t in range(VOCAB) if all(t not in c for c in free_out))
    cache = lm.new_cache(4 * (MAX_LEN // BS), BS)
    nb = cache.free_blocks
    with torch.no_grad():
        everything = TokenFSM.from_allowed(range(VOCAB), vocab=VOCAB)
        assert lm.generate_guided(prompts, everything, N_NEW, cache=cache) == free_out
        assert lm.generate_guided(prompts, [everything, None, everything, None], N_NEW, eos_token_id=eos, cache=cache) == free_out
        fsms = _choices(free_out)
        got = lm.generate_guided(prompts, fsms, N_NEW, eos_token_id=eos, cache=cache)
        print("choices", got)
        assert got == [c[:6] for c in free_out] and all(len(o) == 6 and eos not in o and f.accepts(o) for f, o in zip(fsms, got))
        # a forbidden token: the free run's second most probable token of that step is drawn in its place
        f = _without(free_out)
        got = lm.generate_guided(prompts[:1], f, N_NEW, cache=cache)[0]
        second = int(free_recs[0].top_ids[3, 1])
        print("forbidden", free_out[0][3], "second", second, "got", got)
        assert free_recs[0].top_ids[3, 0] == free_out[0][3] and second != free_out[0][3]
        assert got[:3] == free_out[0][:3] and got[3] == second and len(got) == N_NEW and f.accepts(got)
        # the records show the masked row: the forbidden token has log-probability -inf there and the drawn one rank 1
        toks, recs = lm.generate_guided(prompts[:1], f, N_NEW, logprobs=2, cache=cache)
        assert toks[0] == got and recs[0].rank[3] == 1 and recs[0].top_ids[3, 0] == second and free_out[0][3] not in recs[0].top_ids[3].tolist()
    assert cache.free_blocks == nb


def test_the_guided_loop_equals_the_host_path(lm, prompts, free):
    from qqq_amd import TokenFSM

    free_out, _ = free
    eos = next(t for t in range(VOCAB) if all(t not in c for c in free_out))
    fsms = _choices(free_out)
    mixed = [fsms[0], None, _without(free_out[2:]), fsms[3]]
    with torch.no_grad():
        want_mixed = lm.generate_guided(prompts, mixed, N_NEW, eos_token_id=eos)
        assert want_mixed[0] == free_out[0][:6] and want_mixed[1] == free_out[1] and want_mixed[2][3] != free_out[2][3]
        eager, c_e = _loop(lm, False)
        nb = c_e.free_blocks
        assert eager.generate_guided(prompts, fsms, N_NEW, eos_token_id=eos) == [c[:6] for c in free_out]
        assert eager.generate_guided(prompts, mixed, N_NEW, eos_token_id=eos) == want_mixed and c_e.free_blocks == nb
        graph, c_g = _loop(lm, True)
        for _ in range(2):  # the same graph, the automaton written per call
            assert graph.generate_guided(prompts, fsms, N_NEW, eos_token_id=eos) == [c[:6] for c in free_out]
        assert graph.generate_guided(prompts, mixed, N_NEW, eos_token_id=eos) == want_mixed
        assert graph.generate_guided(prompts, TokenFSM.from_allowed(range(VOCAB), vocab=VOCAB), N_NEW) == free_out
        assert graph.generate(prompts, N_NEW) == free_out  # no automaton: the ops ride along
        assert graph.captures == 1 and eager.captures == 0 and c_g.free_blocks == nb
        assert (graph.remaining == 0).all() and graph.n_fsm.tolist() == graph.n_out.tolist()
        assert lm.generate_guided(prompts, mixed, N_NEW, eos_token_id=eos, device_loop=True) == want_mixed
    for f, o in zip(mixed, want_mixed):
        assert f is None or f.accepts(o, eos=eos)


def test_penalties_records_and_stops_ride_along(lm, prompts, free):
    """every feature of the step at once: the choice free[i][:4] is a proper prefix of free[i][:8], and a min_new_tokens of 6 bans the eos at
    its end, so every completion runs on to eight tokens (the penalties may move it off the free run: the host path is the expectation)"""
    from qqq_amd import TokenFSM

    free_out, _ = free
    eos = next(t for t in range(VOCAB) if all(t not in c for c in free_out))
    fsms = [TokenFSM.from_choices([c[:4], c[:8], c[:2] + [(c[2] + 1) % VOCAB, 5]], vocab=VOCAB) for c in free_out]
    kw = dict(eos_token_id=eos, min_new_tokens=6, stop=[[VOCAB - 1, VOCAB - 2]], repetition_penalty=1.1, presence_penalty=0.1)
    with torch.no_grad():
        short = lm.generate_guided(prompts, fsms, N_NEW, eos_token_id=eos)
        assert all(f.accepts(o, eos=eos) for f, o in zip(fsms, short))
        toks, recs = lm.generate_guided(prompts, fsms, N_NEW, logprobs=2, **kw)
        print("short", short, "toks", toks)
        assert all(f.accepts(o, eos=eos) and len(o) >= 6 for f, o in zip(fsms, toks))
        loop, cache = _loop(lm, True, penalties=True, logprobs=2, stops=True)
        nb = cache.free_blocks
        toks_l, recs_l = loop.generate_guided(prompts, fsms, N_NEW, **kw)
        assert toks_l == toks and cache.free_blocks == nb
        worst = 0.0
        for t, r, rl in zip(toks, recs, recs_l):
            assert r.logprob.shape == rl.logprob.shape == (len(t),) and r.rank.tolist() == rl.rank.tolist()
            assert r.top_ids.tolist() == rl.top_ids.tolist()
            for a, b in ((r.logprob, rl.logprob), (r.top_logprobs, rl.top_logprobs)):
                assert (torch.isinf(a) == torch.isinf(b)).all()
                fin = ~torch.isinf(a)
                worst = max(worst, float((a[fin] - b[fin]).abs().max()) if fin.any() else 0.0)
        print("largest difference of a log-probability between the host path and the loop:", worst)
        # the two paths run the attention at other batch sizes and split plans: their fp16 logits (|l| < 8 here, one ulp 2^-7) may differ
        # by a rounding, and a log-probability moves by at most twice the largest change of a logit
        assert worst <= 2.0 ** -6


def test_a_sampled_run_yields_only_accepted_completions(lm, prompts, free, dev):
    from qqq_amd import TokenFSM

    free_out, _ = free
    eos = next(t for t in range(VOCAB) if all(t not in c for c in free_out))
    fsms = [TokenFSM.from_choices([c[:6], c[:3], c[:2] + [(c[2] + 1) % VOCAB, 1, 2, 3], [7, 8, 9], [7, 9]], vocab=VOCAB) for c in free_out]
    with torch.no_grad():
        host = lm.generate_guided(prompts, fsms, N_NEW, temperature=1.0, eos_token_id=eos, n=2, generator=torch.Generator(device=dev).manual_seed(3))
        loop, cache = _loop(lm, True)
        nb = cache.free_blocks
        looped = loop.generate_guided(prompts, fsms, N_NEW, temperature=1.0, eos_token_id=eos, generator=torch.Generator(device=dev).manual_seed(3))
    print("sampled", host, looped)
    assert all(f.accepts(o, eos=eos) for f, fam in zip(fsms, host) for o in fam)
    assert all(f.accepts(o, eos=eos) for f, o in zip(fsms, looped)) and cache.free_blocks == nb
