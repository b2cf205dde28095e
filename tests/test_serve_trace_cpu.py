"""DecodeLoop's and SpecDecodeLoop's scheduling, event by event, against a trace recorded from the commit before SpecDecodeLoop came to
inherit DecodeLoop.generate (tests/golden/serve_trace.json names that commit): what every forward pass saw of the pool and the state
arrays, every row's tick and the refills of u at every advance, and how the call left the outputs, the pool and the loop.  The forward
pass and the sampler ops are the host stubs of tests/test_step_cpu.py and tests/test_spec_cpu.py.

    python tests/test_serve_trace_cpu.py --write     records the fixture from the qqq_amd/serve.py of the working tree: only ever run
                                                     with the serve.py of the commit named in PARENT checked out"""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "serve_trace.json")
PARENT = "4a340c6"  # the last commit with two generate() methods

PROMPTS = {"plain": [[1, 2, 3], [10] * 17, [20] * 30, [7], [30, 31]],  # budgets of 1, 2, 3, 1 and 1 blocks at 9 new tokens, in both loops:
           "spec": [[1, 2, 3], [0] * 17, [2] * 27, [4], [3, 4]]}       # the third prompt waits for blocks, the last two for a row
# 2 rows and blocks of 16 keys throughout; `eos` fires in the middle of two sequences (plain) / of four and at the first token of one (spec)
SCENARIOS = {
    "greedy": dict(blocks=6, new=9),
    "eos": dict(blocks=6, new=9, eos={"plain": 13, "spec": 1}),
    "sampled": dict(blocks=6, new=9, temperature=1.0, seed=5),
    "refused": dict(blocks=4, new=4, reserved=33, prompts={"plain": [[1] * 3, [2] * 20], "spec": [[1] * 3, [2] * 12]}),
    "one_token": dict(blocks=6, new=1),
}
KEYS = [f"{kind}/{name}" for kind in ("plain", "spec") for name in SCENARIOS]


def _trace(kind, name, monkeypatch):
    import test_spec_cpu
    import test_step_cpu
    from qqq_amd import DecodeLoop, SpecDecodeLoop, serve

    sc = SCENARIOS[name]
    if kind == "plain":
        m = test_step_cpu._tiny_lm()
        test_step_cpu._LoopStub(m, monkeypatch)
        cache = m.new_cache(sc["blocks"], 16)
        loop, op = DecodeLoop(m, cache, rows=2, max_len=48, sync_every=3, u_stride=4, graph=False), "sample_advance"
    else:
        m = test_spec_cpu._tiny_lm()
        test_spec_cpu._LoopStub(m, monkeypatch)
        cache = m.new_cache(sc["blocks"], 16)
        loop, op = SpecDecodeLoop(m, cache, rows=2, max_len=48, draft_len=3, sync_every=3, graph=False), "spec_advance"
    if "reserved" in sc:
        cache.add("other")
        cache.reserve("other", sc["reserved"])
    events, seen = [], dict(u=loop.u.clone(), refills=0)
    forward, advance = m.forward, getattr(serve.ops, op)

    def traced_forward(ids, cache, step, all_rows=False):
        ev = dict(kind="step" if step is loop.step else "prefill", counts=list(step.counts), free_blocks=cache.free_blocks)
        if step is loop.step:
            ev.update(ids=loop.ids.tolist(), pos=loop.pos.tolist(), slots=loop.slots.tolist())
            if kind == "spec":
                ev["start"] = loop.start.tolist()
        events.append(ev)
        return forward(ids, cache, step, all_rows=all_rows)

    def traced_advance(logits, T, k, p, u, tick, *state):
        if not torch.equal(u, seen["u"]):  # a refill shows as other contents; the variates themselves are not recorded
            seen["u"], seen["refills"] = u.clone(), seen["refills"] + 1
        events.append(dict(kind="advance", tick=tick.tolist(), refills=seen["refills"]))
        return advance(logits, T, k, p, u, tick, *state)

    monkeypatch.setattr(m, "forward", traced_forward)
    monkeypatch.setattr(f"qqq_amd.serve.ops.{op}", traced_advance)
    out = error = None
    gen = torch.Generator().manual_seed(sc["seed"]) if "seed" in sc else None
    try:
        out = loop.generate(sc.get("prompts", PROMPTS)[kind], sc["new"], temperature=sc.get("temperature", 0.0), generator=gen,
                            eos_token_id=sc.get("eos", {}).get(kind))
    except Exception as e:  # noqa: BLE001 -- the refusal is part of the trace
        error = [type(e).__name__, str(e)]
    end = dict(out=out, error=error, free_blocks=cache.free_blocks, remaining=loop.remaining.tolist(), ids=loop.ids.tolist(),
               pos=loop.pos.tolist(), slots=loop.slots.tolist(), start=loop.start.tolist() if kind == "spec" else None,
               accepted=getattr(loop, "accepted", None), row_steps=getattr(loop, "row_steps", None), steps=getattr(loop, "steps", None))
    return dict(events=events, end=end)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_names_its_commit_and_holds_every_scenario(recorded):
    assert recorded["parent"] == PARENT and sorted(recorded["traces"]) == sorted(KEYS)
    for kind in ("plain", "spec"):
        tr = recorded["traces"]
        advances = [e for e in tr[f"{kind}/sampled"]["events"] if e["kind"] == "advance"]
        assert advances[0]["refills"] == 1 and advances[-1]["refills"] >= 2  # the call's own variates from its first step on, and a refill
        assert max(max(e["tick"]) for e in advances) >= 1
        assert tr[f"{kind}/refused"]["end"]["error"][0] == "RuntimeError" and "cannot hold a prompt" in tr[f"{kind}/refused"]["end"]["error"][1]
        assert [e["kind"] for e in tr[f"{kind}/refused"]["events"]].count("prefill") == 1  # the first prompt ran, the second never did
        assert tr[f"{kind}/one_token"]["events"] and all(e["kind"] == "prefill" for e in tr[f"{kind}/one_token"]["events"])
        eos = tr[f"{kind}/eos"]["end"]["out"]
        assert any(1 < len(o) < 9 for o in eos) and all(len(o) == 9 for o in tr[f"{kind}/greedy"]["end"]["out"])
        kinds = [e["kind"] for e in tr[f"{kind}/greedy"]["events"]]
        assert kinds.index("step") < len(kinds) - 1 - kinds[::-1].index("prefill")  # a prompt joined after the loop had begun to step


@pytest.mark.parametrize("key", KEYS)
def test_loop_schedules_as_the_recorded_parent_did(recorded, monkeypatch, key):
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
