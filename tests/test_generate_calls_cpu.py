"""What a generate() call does, event by event, on the host path, in DecodeLoop and in SpecDecodeLoop, against a trace recorded from the
commit before the three paths came to share one request object and one first-token routine (tests/golden/generate_calls.json names that
commit): every forward pass with what it saw of the pool, every launch of a sampling op with its logits row count (ops.ban_tokens with
its base), every torch.rand with its shape, and how the call left the tokens, the records, the pool and the loop.  The forward pass and
the ops are the host stubs of tests/test_step_cpu.py, test_spec_cpu.py, test_penalty_cpu.py, test_logprobs_cpu.py and test_stop_cpu.py.

    python tests/test_generate_calls_cpu.py --write     records the fixture from the qqq_amd of the working tree: only ever run with the
                                                         model.py and serve.py of the commit named in PARENT checked out"""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)
FIXTURE = os.path.join(ROOT, "tests", "golden", "generate_calls.json")
PARENT = "f516dfa"  # the last commit with the checks, the first-token pipeline and result() written once per path

# the stub models continue t with t + 1, modulo 50 (host, decode) and modulo 5 (spec, a period the drafter finds).  Blocks of 16 keys, 9
# new tokens, 2 rows: budgets of 1, 2, 1 and 1 blocks through a pool of 3 -- the third prompt waits for blocks (and, in a loop, for a row)
PROMPTS = {"host": [[1, 2, 3], [10] * 17, [7], [20, 21]], "spec": [[1, 2, 3], [0] * 17, [4], [3, 4]]}
PROMPTS["decode"] = PROMPTS["host"]
PENALTIES = dict(repetition_penalty=1.5, presence_penalty=2.0)
# [7, 8] cuts the first prompt's run 4, 5, 6, 7, 8; eos 23 is banned below the minimum in the last prompt's, which goes 22, 0, 1, 2, 3
STOPS = {"host": dict(stop=[[7, 8], [14, 15, 16], [2, 3]], stop_token_ids=[12], min_new_tokens=3, eos_token_id=23),
         "spec": dict(stop=[[1, 2]], stop_token_ids=[3], min_new_tokens=3, eos_token_id=4)}  # 4 banned: 0, 1, 2, cut inside a step
STOPS["decode"] = STOPS["host"]
# with n = 2 a family takes 2, 3, 2 and 2 blocks: the second prompt waits in a pool of 4
SCENARIOS = {
    "plain": dict(),
    "eos": dict(eos={"host": 13, "decode": 13, "spec": 1}),
    "sampled": dict(temperature=1.0, seed=5),
    "penalties": dict(penalties=True),
    "n2": dict(n=2, blocks=4),
    "logprobs": dict(logprobs=2),
    "stops": dict(stops=True),
    "all": dict(n=2, blocks=4, penalties=True, logprobs=2, stops=True),
}
SPEC_SCENARIOS = {name: sc for name, sc in SCENARIOS.items() if name not in ("n2", "logprobs", "all")}
SPEC_SCENARIOS["all"] = dict(penalties=True, stops=True)  # the speculative loop takes neither families nor records
KEYS = [f"{path}/{name}" for path in ("host", "decode", "spec") for name in (SPEC_SCENARIOS if path == "spec" else SCENARIOS)]
OPS = ("penalize_logits", "ban_tokens", "sample_tokens", "topk_logprobs", "topk_logprobs_step", "sample_advance", "spec_advance", "stop_check")


def _records(recs, k):
    if isinstance(recs, list):
        return [_records(r, k) for r in recs]
    return dict(shapes=[list(t.shape) for t in recs], rank=recs.rank.tolist(), token=recs.top_ids[:, 0].tolist() if k else None)


def _flat(tokens):
    """the completions of a call, whether it nests them by n or not"""
    return [c for o in tokens for c in o] if tokens and tokens[0] and isinstance(tokens[0][0], list) else tokens


def _trace(path, name, monkeypatch):
    import test_spec_cpu
    import test_step_cpu
    from qqq_amd import DecodeLoop, SpecDecodeLoop, ops
    from test_logprobs_cpu import _stub_topk, _stub_topk_step
    from test_penalty_cpu import _stub_penalize
    from test_stop_cpu import _stub_ban, _stub_check

    sc = (SPEC_SCENARIOS if path == "spec" else SCENARIOS)[name]
    t = test_spec_cpu if path == "spec" else test_step_cpu
    m = t._tiny_lm()
    t._LoopStub(m, monkeypatch)  # the forward pass, sample_tokens and the loop's advance
    for op, stub in (("penalize_logits", _stub_penalize([])), ("ban_tokens", _stub_ban([])), ("stop_check", _stub_check([])),
                     ("topk_logprobs", _stub_topk([])), ("topk_logprobs_step", _stub_topk_step([]))):
        monkeypatch.setattr(ops, op, stub)
    cache = m.new_cache(sc.get("blocks", 3), 16)
    n, k = sc.get("n", 1), sc.get("logprobs")
    flags = dict(**(dict(penalties=True) if "penalties" in sc else {}), **(dict(family=n) if n > 1 else {}),
                 **(dict(logprobs=k) if k is not None else {}), **(dict(stops=True) if "stops" in sc else {}))
    loop = None
    if path == "decode":
        loop = DecodeLoop(m, cache, rows=2, max_len=48, sync_every=3, u_stride=4, graph=False, **flags)
    elif path == "spec":
        loop = SpecDecodeLoop(m, cache, rows=2, max_len=48, draft_len=3, sync_every=3, graph=False, **flags)

    events = []
    forward, rand = m.forward, torch.rand

    def traced_forward(ids, cache, step, all_rows=False):
        step_pass = step is loop.step if loop is not None else any(s > 0 for s in step.starts)
        events.append(dict(kind="step" if step_pass else "prefill", counts=list(step.counts), free_blocks=cache.free_blocks))
        return forward(ids, cache, step, all_rows=all_rows)

    def traced(op, f):
        def call(first, *a, **kw):
            events.append(dict(kind=op, rows=first.shape[0], **(dict(base=kw.get("base", 0)) if op == "ban_tokens" else {})))
            return f(first, *a, **kw)
        return call

    def traced_rand(*shape, **kw):
        events.append(dict(kind="rand", shape=list(shape[0]) if isinstance(shape[0], (tuple, list)) else list(shape)))
        return rand(*shape, **kw)

    monkeypatch.setattr(m, "forward", traced_forward)
    for op in OPS:
        monkeypatch.setattr(ops, op, traced(op, getattr(ops, op)))
    monkeypatch.setattr(torch, "rand", traced_rand)
    kw = dict(temperature=sc.get("temperature", 0.0), generator=torch.Generator().manual_seed(sc["seed"]) if "seed" in sc else None)
    if "eos" in sc:
        kw["eos_token_id"] = sc["eos"][path]
    if "penalties" in sc:
        kw.update(PENALTIES)
    if "stops" in sc:
        kw.update(STOPS[path])
    if loop is None:
        got = m.generate(PROMPTS[path], 9, cache=cache, **kw, **(dict(n=n) if n > 1 else {}), **(dict(logprobs=k) if k is not None else {}))
    else:
        got = loop.generate(PROMPTS[path], 9, **kw)
    tokens, recs = got if k is not None else (got, None)
    end = dict(tokens=tokens, records=None if recs is None else _records(recs, k), free_blocks=cache.free_blocks)
    if loop is not None:
        end.update(remaining=loop.remaining.tolist(), pos=loop.pos.tolist(), n_out=loop.n_out.tolist())
    return dict(events=events, end=end)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_names_its_commit_and_its_scenarios_reach_what_they_are_for(recorded):
    assert recorded["parent"] == PARENT and sorted(recorded["traces"]) == sorted(KEYS)
    tr = recorded["traces"]
    for path in ("host", "decode", "spec"):
        kinds = [e["kind"] for e in tr[f"{path}/plain"]["events"]]
        assert kinds.index("step") < len(kinds) - 1 - kinds[::-1].index("prefill")  # a prompt waited, and joined after the first step
        assert tr[f"{path}/plain"]["end"]["free_blocks"] == 3 and all(len(o) == 9 for o in tr[f"{path}/plain"]["end"]["tokens"])
        assert any(1 < len(o) < 9 for o in tr[f"{path}/eos"]["end"]["tokens"])
        assert any(e["kind"] == "rand" for e in tr[f"{path}/sampled"]["events"])
        for name in ("plain", "eos", "sampled"):
            assert {e["kind"] for e in tr[f"{path}/{name}"]["events"]} <= {"prefill", "step", "rand", "sample_tokens", "sample_advance", "spec_advance"}
        assert any(e["kind"] == "penalize_logits" for e in tr[f"{path}/penalties"]["events"])
        for name in ("stops", "all"):
            assert any(e["kind"] == "ban_tokens" and e["base"] == 0 for e in tr[f"{path}/{name}"]["events"])
            assert any(len(o) < 9 for o in _flat(tr[f"{path}/{name}"]["end"]["tokens"]))  # a completion ended on a stop
    for path in ("host", "decode"):
        assert all(len(o) == 2 for o in tr[f"{path}/n2"]["end"]["tokens"])
        assert any(e["kind"] == "topk_logprobs" for e in tr[f"{path}/logprobs"]["events"])
        for toks, recs in zip(tr[f"{path}/logprobs"]["end"]["tokens"], tr[f"{path}/logprobs"]["end"]["records"]):
            assert recs["token"] == toks and recs["shapes"] == [[len(toks)], [len(toks)], [len(toks), 2], [len(toks), 2]]


@pytest.mark.parametrize("key", KEYS)
def test_generate_calls_what_the_recorded_parent_called(recorded, monkeypatch, key):
    got = json.loads(json.dumps(_trace(*key.split("/"), monkeypatch)))
    want = recorded["traces"][key]
    for n, (g, w) in enumerate(zip(got["events"], want["events"])):
        assert g == w, f"{key}: event {n} differs"
    assert len(got["events"]) == len(want["events"])
    assert got["end"] == want["end"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    traces = {}
    for key in KEYS:
        with pytest.MonkeyPatch.context() as mp:
            traces[key] = _trace(*key.split("/"), mp)
    with open(FIXTURE, "w") as f:  # a trace per line
        f.write('{"parent": "%s", "traces": {\n' % PARENT)
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in traces.items()))
        f.write("\n}}\n")
    print(f"wrote {FIXTURE}: {os.path.getsize(FIXTURE)} bytes")
