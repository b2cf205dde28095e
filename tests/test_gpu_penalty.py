"""ops.penalize_logits on the GPU against tests/penalty_ref.py, bit for bit on the logits (their padding columns included) AND on `seen`,
with the workspace all zero afterwards and no other input changed; every test sends at least two calls on fresh inputs through one
workspace.  Shapes, history lengths around a lane, a wave, a workgroup and two passes of it, the contents the rule distinguishes, the
special values, idle and neutral rows, replay from a captured graph, and the composition with ops.sample_tokens."""
import numpy as np
import pytest
import torch

import penalty_ref

pytestmark = pytest.mark.gpu

f16, f32, i32, i64 = np.float16, np.float32, np.int32, np.int64
SENTINEL = 0x5a5a  # the bits of the padding columns vocab ... ld - 1
LENGTHS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)  # p + 1: one lane, a wave +- 1, a workgroup of any size up to 1024 +- 1, > 2 passes
# +, -, +-0, +-inf, NaN of either sign, the largest finite values and +-60000 (whose penalised results leave fp16), the smallest denormals
SPECIALS = np.array([0x0000, 0x8000, 0x7c00, 0xfc00, 0x7e00, 0xfe00, 0x7bff, 0xfbff, 0x7b53, 0xfb53, 0x0001, 0x8001, 0x4400, 0xc400], np.uint16)
# each of the three alone, all three, a repetition penalty below 1 (60000 / 0.5 overflows) and presence / frequency that overflow
PARAMS = ((1.3, 0.0, 0.0), (1.0, 0.5, 0.0), (1.0, 0.0, 0.25), (1.3, 0.5, 0.25), (0.5, -0.5, 0.125), (1.0, 3e4, 3e4))


def _case(rng, rows, vocab, ld, g, lens, n_prompt=None, params=None, tokens="mixed", stride=None):
    """Inputs of one call: row r has a history of lens[r] tokens (0: an idle row, pos -1).  tokens: "mixed" -- uniform over [-1, vocab],
    both ends outside the vocabulary, with drafts that repeat history tokens and each other; "distinct" -- no token twice; "same" -- one
    token throughout, the drafts too."""
    m = rows * g
    stride = stride or max(max(lens), 1) + 3
    logits = (rng.standard_normal((m, ld)) * 4).astype(f16)
    seen = rng.integers(0, vocab, (rows, stride)).astype(i32)  # what lies at and behind p is never read
    ids = np.zeros((rows, g), i64)
    pos = np.full((rows, g), -1, i64)
    for r, n in enumerate(lens):
        if tokens == "distinct":
            perm = rng.permutation(vocab)[:n + g - 1]
            h, d = perm[:n], perm[n:]
        elif tokens == "same":
            h, d = np.full(n, r % vocab), np.full(g - 1, r % vocab)
        else:
            h = rng.integers(-1, vocab + 1, n)
            d = rng.integers(-1, vocab + 1, g - 1)
            if n >= 3:
                h[rng.choice(n, 2, replace=False)] = [-1, vocab]
            for k in range(g - 1):  # a draft that is a history token, and the same token twice among the drafts
                if n and rng.random() < 0.4:
                    d[k] = h[rng.integers(n)]
                elif k and rng.random() < 0.4:
                    d[k] = d[rng.integers(k)]
        if n:
            seen[r, :n - 1] = h[:-1]
            ids[r, 0] = h[-1]
            pos[r] = n - 1 + np.arange(g)
        ids[r, 1:] = d
        cols = np.unique(np.concatenate([h[:48], h[-16:], d]))
        cols = cols[(cols >= 0) & (cols < vocab)]
        for j in range(g):  # special values where the rule acts, and a few where it does not
            at = np.concatenate([cols[rng.random(cols.size) < 0.5], rng.integers(0, vocab, 4)]).astype(np.int64)
            logits[r * g + j, at] = rng.choice(SPECIALS, at.size).view(f16)
    logits.view(np.uint16)[:, vocab:] = SENTINEL
    if n_prompt is None:  # none, some, all of the history, and past the drafts
        n_prompt = [int(rng.choice([0, n // 2, n, n + 2 * g])) for n in lens]
    if params is None:
        params = [PARAMS[int(rng.integers(len(PARAMS)))] for _ in lens]
    rep, pres, freq = (np.array([p[i] for p in params], f32) for i in range(3))
    if g == 1:
        ids, pos = ids[:, 0].copy(), pos[:, 0].copy()  # the decode loop's arrays are [rows]
    return dict(logits=logits, ids=ids, pos=pos, seen=seen, n_prompt=np.array(n_prompt, i32), rep=rep, pres=pres, freq=freq, vocab=vocab)


def _to_dev(c, dev):
    d = {k: torch.from_numpy(v).to(dev) for k, v in c.items() if k != "vocab"}
    d["view"] = d["logits"][:, :c["vocab"]]
    return d


def _expect(c):
    return penalty_ref.penalize(c["logits"], c["ids"], c["pos"], c["seen"], c["n_prompt"], c["rep"], c["pres"], c["freq"], c["vocab"])


def _compare(c, d, ws, what=""):
    want_logits, want_seen = _expect(c)
    got = d["logits"].cpu().numpy().view(np.uint16)
    want = want_logits.view(np.uint16)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), [(int(a), int(b), hex(int(c["logits"].view(np.uint16)[a, b])), hex(int(got[a, b])), hex(int(want[a, b])))
                                            for a, b in bad[:6]])
    assert np.array_equal(d["seen"].cpu().numpy(), want_seen), what
    assert int(torch.count_nonzero(ws)) == 0, what
    for k in ("ids", "pos", "n_prompt", "rep", "pres", "freq"):
        assert np.array_equal(d[k].cpu().numpy(), c[k], equal_nan=k in ("rep", "pres", "freq")), (what, k)


def _check(dev, cases):
    """every case through ONE workspace, call after call"""
    from qqq_amd import ops

    ws = torch.zeros(max(c["ids"].shape[0] * c["vocab"] for c in cases), dtype=torch.int32, device=dev)
    for n, c in enumerate(cases):
        d = _to_dev(c, dev)
        out = ops.penalize_logits(d["view"], d["ids"], d["pos"], d["seen"], d["n_prompt"], d["rep"], d["pres"], d["freq"], ws)
        torch.cuda.synchronize()
        assert out is d["view"]
        _compare(c, d, ws, f"call {n}")


def _lengths(rows, calls_at_least=2):
    """history lengths for as many calls of `rows` rows as cover LENGTHS, longest first"""
    order = sorted(LENGTHS, reverse=True)
    calls = max(calls_at_least, -(-len(order) // rows))
    return [[order[(c * rows + r) % len(order)] for r in range(rows)] for c in range(calls)]


# ---- 1. shapes x history lengths, mixed contents, every parameter set

@pytest.mark.parametrize("rows,vocab,ld,g", [(1, 7, 8, 1), (5, 7, 8, 3), (5, 7, 8, 16), (5, 1000, 1000, 1), (1, 1000, 1008, 3), (5, 1000, 1008, 3),
                                             (1, 1000, 1000, 16), (5, 1000, 1008, 16), (2, 262144, 262144, 1), (2, 262144, 262152, 3)])
def test_shapes_and_history_lengths(dev, rows, vocab, ld, g):
    rng = np.random.default_rng(rows * 1000003 + vocab * 31 + ld + g)
    lens = _lengths(rows)
    if g == 16:  # the reference's cost is history x G: the long histories ride with G = 1 and 3
        lens = [[min(n, 65 + r) for r, n in enumerate(row)] for row in lens]
    assert g == 16 or {n for row in lens for n in row} == set(LENGTHS)
    _check(dev, [_case(rng, rows, vocab, ld, g, row) for row in lens])


# ---- 2. the contents the rule distinguishes

@pytest.mark.parametrize("g", [1, 3])
def test_all_distinct_and_all_the_same_token(dev, g):
    """2049 distinct tokens (each word of the workspace touched once) and 2049 times one token (one contended word, c = 2049 - n_prompt),
    under every parameter set and with the prompt ending nowhere, inside, at the end of the history and past the drafts."""
    rng = np.random.default_rng(40 + g)
    vocab, cases = 4099, []
    for kind in ("distinct", "same"):
        for n_prompt in ([0, 5], [2049, 2049 + 2 * g], [1024, 2050]):
            cases.append(_case(rng, 2, vocab, vocab + 5, g, [2049, 2049], n_prompt=n_prompt, tokens=kind,
                               params=[PARAMS[len(cases) % len(PARAMS)], PARAMS[3]]))
    _check(dev, cases)
    # the count that reaches the rule: 2049 - 5 outputs of the one token, plus the drafts in front of a logits row
    c = cases[3]
    want, _ = _expect(c)
    r, t = 1, 1
    for j in range(g):
        assert want[r * g + j, t].view(np.uint16) == penalty_ref.rule(c["logits"][r * g + j, t], 2049 - 5 + j, *PARAMS[3]).view(np.uint16)


def test_hand_built_rows(dev):
    """One row per content: a token in prompt and output; a token only in the drafts; the same token twice among the drafts; -1 and vocab
    in seen and in ids; a draft that repeats the row's last token; drafts at prompt indices.  vocab 1000 in rows of 1008, G = 4."""
    rng = np.random.default_rng(7)
    vocab, ld, g = 1000, 1008, 4
    hist = [[5, 6, 7, 5, 8, 5], [1, 2, 3], [1, 2, 3], [-1, 4, vocab, 4, -1], [9, 9, 9], [10, 11, 12, 13], [20]]
    ids0 = [5, 3, 3, vocab, 9, 13, -1]
    drafts = [[6, 6, 100], [400, 2, 401], [500, 500, 500], [-1, vocab, 4], [9, 9, 10], [11, 14, 11], [vocab, 20, -1]]
    n_prompt = [2, 3, 0, 1, 1, 9, 0]
    cases = []
    for params in (PARAMS[3], PARAMS[0], PARAMS[1], PARAMS[2]):
        c = _case(rng, len(hist), vocab, ld, g, [len(h) for h in hist], n_prompt=n_prompt, params=[params] * len(hist))
        for r, h in enumerate(hist):
            c["seen"][r, :len(h) - 1] = h[:-1]
            c["ids"][r] = [ids0[r]] + drafts[r]
        cases.append(c)
    # spot checks of the reference itself, on values computed by hand from the rule
    c = cases[0]
    want, seen = _expect(c)
    L = lambda r, j, t: c["logits"][r * g + j, t]  # noqa: E731
    rule = lambda l, n: penalty_ref.rule(l, n, *PARAMS[3]).view(np.uint16)  # noqa: E731
    W = lambda r, j, t: want[r * g + j, t].view(np.uint16)  # noqa: E731
    assert W(0, 0, 5) == rule(L(0, 0, 5), 2) and W(0, 0, 6) == rule(L(0, 0, 6), 0)        # 5: a prompt and two output occurrences; 6: prompt only
    assert W(0, 1, 6) == rule(L(0, 1, 6), 1) and W(0, 2, 6) == rule(L(0, 2, 6), 2)        # the draft 6 once, then twice
    assert W(0, 2, 100) == L(0, 2, 100).view(np.uint16) and W(0, 3, 100) == rule(L(0, 3, 100), 1)  # only in the last draft
    assert W(1, 0, 400) == L(1, 0, 400).view(np.uint16) and W(1, 1, 400) == rule(L(1, 1, 400), 1)
    assert W(2, 3, 500) == rule(L(2, 3, 500), 3) and W(5, 3, 11) == rule(L(5, 3, 11), 0)  # drafts at prompt indices count as prompt tokens
    assert seen[3, 4] == -1 and seen[6, 0] == -1 and seen[0, 5] == 5
    _check(dev, cases)


# ---- 3. idle, guarded and neutral rows; the padding

def test_idle_guarded_and_neutral_rows(dev):
    """Row 0 idle (pos -1), row 1 at p == seen_stride, row 2 at p > seen_stride: nothing of them changes in any array.  Rows 3 and 4 neutral
    (1, 0, 0 and 1, -0, 0): recorded in seen, their logits -- NaN payloads included -- keep their bits.  Row 5 works."""
    from qqq_amd import ops

    rng = np.random.default_rng(11)
    vocab, ld, stride = 1000, 1008, 40
    for g in (1, 3):
        cases = []
        for _ in range(2):
            c = _case(rng, 6, vocab, ld, g, [0, 30, 30, 30, 17, 40], stride=stride,
                      params=[PARAMS[3], PARAMS[3], PARAMS[3], (1.0, 0.0, 0.0), (1.0, -0.0, 0.0), PARAMS[3]])
            pos = c["pos"].reshape(6, -1)
            pos[1], pos[2] = stride + np.arange(g), stride + 7 + np.arange(g)
            c["logits"].view(np.uint16)[3 * g:5 * g, :64] = rng.integers(0x7c01, 0x8000, (2 * g, 64))  # NaN of every payload
            cases.append(c)
        _check(dev, cases)
        want, seen = _expect(cases[0])
        assert np.array_equal(want.view(np.uint16)[:5 * g], cases[0]["logits"].view(np.uint16)[:5 * g])
        assert not np.array_equal(want[5 * g:].view(np.uint16), cases[0]["logits"][5 * g:].view(np.uint16))
        t = int(cases[0]["ids"].reshape(6, -1)[3, 0])
        assert np.array_equal(seen[:3], cases[0]["seen"][:3]) and seen[3, 29] == (t if 0 <= t < vocab else -1)
    # floats for the parameters, and a workspace of the op's own
    c = _case(rng, 3, vocab, ld, 1, [5, 64, 9], params=[PARAMS[3]] * 3)
    d = _to_dev(c, dev)
    assert ops.penalize_logits(d["view"], d["ids"], d["pos"], d["seen"], d["n_prompt"], *PARAMS[3]) is d["view"]
    torch.cuda.synchronize()
    _compare(c, d, torch.zeros(1, device=dev), "floats")
    with pytest.raises(RuntimeError, match="never copied"):
        ops.penalize_logits(d["logits"].t()[:vocab].t()[:, ::2], d["ids"], d["pos"], d["seen"], d["n_prompt"], *PARAMS[3])


# ---- 4. replay from a captured graph

@pytest.mark.parametrize("g", [1, 5])
def test_graph_replay_with_other_contents(dev, g):
    from qqq_amd import ops

    rng = np.random.default_rng(70 + g)
    rows, vocab, ld, stride = 5, 1000, 1008, 1100
    first = _case(rng, rows, vocab, ld, g, [1025, 64, 0, 2, 300], stride=stride)
    d = _to_dev(first, dev)
    ws = torch.zeros(rows * vocab, dtype=torch.int32, device=dev)
    call = lambda: ops.penalize_logits(d["view"], d["ids"], d["pos"], d["seen"], d["n_prompt"], d["rep"], d["pres"], d["freq"], ws)  # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream(dev).wait_stream(side)
    for lens in ([3, 0, 1024, 65, 1023], [0, 700, 1, 63, 1100]):  # every input changes, idle rows move
        c = _case(rng, rows, vocab, ld, g, lens, stride=stride)
        for k in d:
            if k != "view":
                d[k].copy_(torch.from_numpy(c[k]))
        graph.replay()
        torch.cuda.synchronize()
        _compare(c, d, ws, f"replay {lens}")


# ---- 5. in front of the sampler

def test_composition_with_sample_tokens(dev):
    from qqq_amd import ops

    rng = np.random.default_rng(5)
    rows, vocab, ld = 5, 1000, 1008
    c = _case(rng, rows, vocab, ld, 1, [64, 300, 0, 1025, 9])
    c["logits"] = (rng.standard_normal((rows, ld)) * 2).astype(f16)  # finite rows: the sampled draws spread
    c["logits"].view(np.uint16)[:, vocab:] = SENTINEL
    want, _ = _expect(c)
    ref = torch.from_numpy(want).to(dev)[:, :vocab]
    u = torch.rand(rows, generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    for T, k, p in ((0.0, 0, 1.0), (0.9, 50, 0.95), (1.5, 0, 1.0)):
        d = _to_dev(c, dev)
        got = ops.sample_tokens(ops.penalize_logits(d["view"], d["ids"], d["pos"], d["seen"], d["n_prompt"], d["rep"], d["pres"], d["freq"]),
                                T, k, p, u)
        assert got.tolist() == ops.sample_tokens(ref, T, k, p, u).tolist(), (T, k, p)
    # the penalties do move the greedy token of a row whose maximum was emitted before (a property of the inputs, asserted)
    plain = ops.sample_tokens(torch.from_numpy(c["logits"]).to(dev)[:, :vocab], 0.0, 0, 1.0, u).tolist()
    top = int(plain[1])
    c["seen"][1, 10] = top
    c["n_prompt"][1], c["rep"][1], c["pres"][1], c["freq"][1] = 0, 1.0, 3e4, 0.0
    d = _to_dev(c, dev)
    moved = ops.sample_tokens(ops.penalize_logits(d["view"], d["ids"], d["pos"], d["seen"], d["n_prompt"], d["rep"], d["pres"], d["freq"]),
                              0.0, 0, 1.0, u).tolist()
    assert moved[1] != top and moved[2] == plain[2]
