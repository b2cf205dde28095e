"""stop, stop_token_ids and min_new_tokens through the three generate paths on the GPU, greedy, on the model and prompts of
tests/test_gpu_model.py: a free run supplies a 2-token stop sequence from inside one completion and a stop id from another, and the
expectation is that run cut in plain Python.  The host path, DecodeLoop (eager and captured, four prompts through three rows) and
SpecDecodeLoop (eager and captured) must all give it; with a minimum length, an eos that ended a completion early is deferred."""
import pytest
import torch

from test_gpu_model import _make_lm, _prompts

pytestmark = pytest.mark.gpu

N_NEW, BS, ROWS, MAX_LEN, K = 12, 16, 3, 64, 3


@pytest.fixture(scope="module")
def lm(dev):
    return _make_lm(dev, 128).fuse_prefill()


@pytest.fixture(scope="module")
def prompts():
    p = _prompts()
    return p + [p[1][::-1][:9]]  # a fourth: one more than the loops have rows


@pytest.fixture(scope="module")
def free(lm, prompts):
    """the free greedy run of the host path, never changed"""
    with torch.no_grad():
        out = lm.generate(prompts, N_NEW)
    assert all(len(o) == N_NEW for o in out)
    return out


def _cut(free, stop=(), stop_token_ids=(), least=0):
    """the completions of a free run as generate() must end them: the rules in plain Python, one length at a time"""
    out = []
    for c in free:
        got = list(c)
        for e in range(1, len(c) + 1):
            if e < least:
                continue
            if c[e - 1] in stop_token_ids:
                got = c[:e]
                break
            hit = next((s for s in stop if len(s) <= e and c[e - len(s):e] == list(s)), None)
            if hit is not None:
                got = c[:e - len(hit)]
                break
        out.append(got)
    return out


def _picks(free):
    stop = free[1][4:6]       # inside completion 1
    stop_id = free[0][7]      # from completion 0
    return [stop], [stop_id]


def _decode_loop(lm, graph, **kw):
    from qqq_amd import DecodeLoop

    cache = lm.new_cache(ROWS * (MAX_LEN // BS), BS)
    return DecodeLoop(lm, cache, rows=ROWS, max_len=MAX_LEN, sync_every=3, graph=graph, stops=True, **kw), cache


def _spec_loop(lm, graph, stops=True):
    from qqq_amd import SpecDecodeLoop

    cache = lm.new_cache(ROWS * (MAX_LEN // BS), BS)
    return SpecDecodeLoop(lm, cache, rows=ROWS, max_len=MAX_LEN, draft_len=K, sync_every=3, graph=graph, stops=stops), cache


def test_the_host_path_cuts_the_first_occurrence(lm, prompts, free):
    stop, ids = _picks(free)
    want = _cut(free, stop, ids)
    print("free", free, "stop", stop, "ids", ids, "want", want)
    assert len(want[1]) <= 4 and len(want[0]) <= 8 and want != free and want[0][-1] == ids[0]
    with torch.no_grad():
        assert lm.generate(prompts, N_NEW, stop=stop) == _cut(free, stop)
        assert lm.generate(prompts, N_NEW, stop_token_ids=ids) == _cut(free, (), ids)
        assert lm.generate(prompts, N_NEW, stop=stop, stop_token_ids=ids) == want
        # a stop on a first token leaves an empty completion; the others are the free run's
        first = [[free[2][0]]]
        assert lm.generate(prompts, N_NEW, stop=first) == _cut(free, first) and _cut(free, first)[2] == []


def test_decode_loop_equals_the_host_path(lm, prompts, free):
    stop, ids = _picks(free)
    want = _cut(free, stop, ids)
    with torch.no_grad():
        eager, c_e = _decode_loop(lm, False)
        nb = c_e.free_blocks
        assert eager.generate(prompts, N_NEW) == free  # the ops ride along with empty tables
        assert eager.generate(prompts, N_NEW, stop=stop, stop_token_ids=ids) == want and c_e.free_blocks == nb
        graph, c_g = _decode_loop(lm, True)
        for _ in range(2):  # the same graph, the tables written per call
            assert graph.generate(prompts, N_NEW, stop=stop, stop_token_ids=ids) == want
        first = [[free[2][0]]]
        assert graph.generate(prompts, N_NEW, stop=first) == _cut(free, first)
        assert graph.generate(prompts, N_NEW) == free
    assert graph.captures == 1 and eager.captures == 0 and c_g.free_blocks == nb
    assert lm.generate(prompts, N_NEW, device_loop=True, stop=stop, stop_token_ids=ids) == want


def test_spec_loop_equals_the_expectation(lm, prompts, free):
    with torch.no_grad():
        plain, _ = _spec_loop(lm, False, stops=False)
        own = plain.generate(prompts, N_NEW)  # the speculative loop's greedy tokens are the host path's up to near-ties of the logits
        print("spec free run equals the host path's:", own == free)
        stop, ids = _picks(own)
        want = _cut(own, stop, ids)
        assert want != own
        eager, c_e = _spec_loop(lm, False)
        nb = c_e.free_blocks
        assert eager.generate(prompts, N_NEW) == own
        assert eager.generate(prompts, N_NEW, stop=stop, stop_token_ids=ids) == want and c_e.free_blocks == nb
        graph, c_g = _spec_loop(lm, True)
        for _ in range(2):
            assert graph.generate(prompts, N_NEW, stop=stop, stop_token_ids=ids) == want
        assert graph.generate(prompts, N_NEW) == own
    assert graph.captures == 1 and c_g.free_blocks == nb
    assert own == free


def test_min_new_tokens_defers_an_eos(lm, prompts, free):
    eos = free[1][2]  # ends completion 1 at three tokens
    with torch.no_grad():
        ended = lm.generate(prompts, N_NEW, eos_token_id=eos)
        assert ended[1] == free[1][:3]
        host = lm.generate(prompts, N_NEW, eos_token_id=eos, min_new_tokens=5)
        print("eos", eos, "host", host)
        for got, was in zip(host, free):
            assert eos not in got[:5] and len(got) >= 5 and (eos not in got or got.index(eos) == len(got) - 1)
            assert got[:2] == was[:2] or eos in was[:2]
        assert host[1][:2] == free[1][:2] and host[1] != ended[1]
        eager, _ = _decode_loop(lm, False)
        graph, _ = _decode_loop(lm, True)
        assert eager.generate(prompts, N_NEW, eos_token_id=eos, min_new_tokens=5) == host
        assert graph.generate(prompts, N_NEW, eos_token_id=eos, min_new_tokens=5) == host
        spec_e, _ = _spec_loop(lm, False)
        spec_g, _ = _spec_loop(lm, True)
        assert spec_e.generate(prompts, N_NEW, eos_token_id=eos, min_new_tokens=5) == host
        assert spec_g.generate(prompts, N_NEW, eos_token_id=eos, min_new_tokens=5) == host
        # the budget wins over the minimum
        assert lm.generate(prompts, 3, eos_token_id=eos, min_new_tokens=5) == [o[:3] for o in host]
        # records: one per token, and the banned eos shows as -inf in the rows below the minimum
        toks, recs = lm.generate(prompts, N_NEW, eos_token_id=eos, min_new_tokens=5, logprobs=5)
        loop, _ = _decode_loop(lm, True, logprobs=5)
        toks_l, recs_l = loop.generate(prompts, N_NEW, eos_token_id=eos, min_new_tokens=5)
        assert toks == host and toks_l == host
        for t, r, rl in zip(toks, recs, recs_l):
            assert r.logprob.shape == rl.logprob.shape == (len(t),) and r.top_ids.shape == rl.top_ids.shape == (len(t), 5)
            assert r.top_ids[:, 0].tolist() == t and rl.top_ids[:, 0].tolist() == t
            assert eos not in r.top_ids[:5].flatten().tolist() and eos not in rl.top_ids[:5].flatten().tolist()
        # ... and are cut with their tokens
        stop, ids = _picks(free)
        toks, recs = lm.generate(prompts, N_NEW, stop=stop, stop_token_ids=ids, logprobs=5)
        toks_l, recs_l = loop.generate(prompts, N_NEW, stop=stop, stop_token_ids=ids)
        assert toks == toks_l == _cut(free, stop, ids)
        assert [len(t) for t in toks] == [r.logprob.shape[0] for r in recs] == [r.logprob.shape[0] for r in recs_l]
        assert all(r.top_ids[:, 0].tolist() == t for t, r in zip(toks, recs_l))


def test_an_eos_goes_before_a_stop_sequence_that_ends_in_it_on_every_path(lm, prompts, free):
    """the row's eos retires the row inside the sampler's step; the check behind it must keep the token where a sequence ends in it --
    as a later token and as the first one, where admission decides"""
    later, first = free[1][3], free[2][0]
    with torch.no_grad():
        loops = [_decode_loop(lm, False)[0], _decode_loop(lm, True)[0], _spec_loop(lm, False)[0], _spec_loop(lm, True)[0]]
        for eos, stop in ((later, [free[1][2:4]]), (later, [[later]]), (first, [[first]]), (later, [free[1][1:3]])):
            want = _cut(free, stop, [eos])  # an eos is a stop id of its own: the rule of _cut
            assert want != free and (eos != later or want[1] in (free[1][:4], free[1][:1])) and (eos != first or want[2] == [first])
            assert lm.generate(prompts, N_NEW, eos_token_id=eos, stop=stop) == want
            for loop in loops:
                assert loop.generate(prompts, N_NEW, eos_token_id=eos, stop=stop) == want, (loop._name, loop.graph, eos, stop)
