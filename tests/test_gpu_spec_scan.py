"""qqq_spec_advance_kernel's drafter scan on the GPU past one wave and one pass: one call of ops.spec_advance over tests/spec_corpus.py --
matches planted at end positions in every wave of the first, the second and a later pass of the scan, competing matches, the cap, the
row's start, the overlapping copy, appends that feed the scan, the table's end, unreachable state and 1500 random histories of up to 1099
tokens -- against tests/spec_ref.py, every field bit for bit.  tests/test_spec_corpus_cpu.py shows that each case is what it is planned
to be and that a scan which picked another of its occurrences would draft other tokens.

The draws are steered as in tests/test_gpu_spec.py: 3 * randn noise with a spike of +40 at the planned token, whose probability is 1 to
within e^-30, greedy or sampled; ops.sample_tokens confirms them."""
import numpy as np
import pytest
import torch

import spec_corpus as sc
import spec_ref

pytestmark = pytest.mark.gpu

LD = 1008
GREEDY, SAMPLED = (0.0, 0, 1.0), (0.8, 50, 0.9)


def _to_dev(st, dev):
    return {k: torch.from_numpy(v).to(dev) for k, v in st.items() if isinstance(v, np.ndarray)}


def _logits(draws, vocab, ld, gen, dev):
    """[rows * G, vocab] inside a buffer of ld columns: noise, and +40 where each draw is to land"""
    m = draws.size
    buf = torch.zeros((m, ld), dtype=torch.float16, device=dev)
    buf[:, :vocab] = (3.0 * torch.randn((m, vocab), generator=gen, device=dev)).half()
    buf[:, vocab:] = float("inf")  # the padding columns are never read
    buf[torch.arange(m, device=dev), torch.from_numpy(draws.reshape(-1)).to(dev)] = 40.0
    return buf


def _params(rows, g, mode, gen, dev):
    return dict(T=torch.full((rows * g,), mode[0], device=dev), k=torch.full((rows * g,), mode[1], dtype=torch.int32, device=dev),
                p=torch.full((rows * g,), mode[2], device=dev), u=torch.rand((rows, 2 * g), generator=gen, device=dev))


def _call(ops, logits, par, d, block_size, nmax):
    ops.spec_advance(logits, par["T"], par["k"], par["p"], par["u"], d["tick"], d["ids"], d["pos"], d["slots"], d["start"], d["block_table"],
                     d["remaining"], d["eos"], d["hist"], d["hist_len"], d["n_out"], d["n_acc"], block_size, nmax)


def _tokens(ops, logits, par, tick, g):
    """ops.sample_tokens on the same logits rows with the variates the call indexes -> [rows, g]"""
    idx = (tick.long()[:, None] * g + torch.arange(g, device=tick.device)[None]) % par["u"].shape[1]
    u = par["u"].gather(1, idx).reshape(-1).contiguous()
    return ops.sample_tokens(logits, par["T"], par["k"], par["p"], u).view(-1, g).cpu().numpy()


def _describe(batch, r):
    case = batch["cases"].get(r)
    if case is None:
        return f"row {r}: an idle sentinel row"
    plan = case["plan"]
    if plan is None:
        return f"row {r}: {case['name']} (no match planned, or the row retires)"
    wave, ps = sc.where(plan["c"])
    return f"row {r}: {case['name']} n {plan['n']} c {plan['c']} wave {wave} pass {plan['c'] // 256} (class {ps})"


def _run_batch(dev, batch, mode, seed, vocab=sc.VOCAB, ld=LD):
    """one call over the batch's state -> the device state behind it; every field is compared with the reference here"""
    from qqq_amd import ops

    st, draws, nmax = batch["state"], batch["draws"], batch["ngram_max"]
    rows, g = draws.shape
    gen = torch.Generator(device=dev).manual_seed(seed)
    par = _params(rows, g, mode, gen, dev)
    logits = _logits(draws, vocab, ld, gen, dev)[:, :vocab]
    d = _to_dev(st, dev)
    toks = _tokens(ops, logits, par, d["tick"], g)
    off = np.argwhere(toks != draws)
    assert off.size == 0, f"draw not steered: {_describe(batch, int(off[0][0]))} draw {int(off[0][1])}"
    _call(ops, logits, par, d, batch["block_size"], nmax)
    torch.cuda.synchronize()
    want = spec_ref.advance(spec_ref.copy_state(st), toks.tolist(), nmax)
    for f in spec_ref.FIELDS:
        got = d[f].cpu().numpy()
        bad = np.flatnonzero((got != want[f]).reshape(rows, -1).any(axis=1))
        groups = sorted({batch["cases"][int(r)]["group"] if int(r) in batch["cases"] else "idle" for r in bad})
        assert bad.size == 0, (f"{f} differs in {bad.size} rows of the groups {groups}; " + "; ".join(
            f"{_describe(batch, int(r))}: got {got[r].tolist()[-20:]} want {want[f][r].tolist()[-20:]}" for r in bad[:4]))
    for f in ("block_table", "eos"):  # only read
        assert np.array_equal(d[f].cpu().numpy(), st[f]), f
    for r in batch["idle"]:  # the sentinel rows: nothing but the tick
        for f in spec_ref.FIELDS:
            assert np.array_equal(d[f][r].cpu().numpy(), st[f][r] + (f == "tick")), (f, r)
    return d


@pytest.fixture(scope="module")
def corpus():
    made = {}

    def get(k, nmax):
        if (k, nmax) not in made:
            made[(k, nmax)] = sc.batches(k, nmax)
        return made[(k, nmax)]

    return get


@pytest.mark.parametrize("k, nmax", sc.PAIRS)
def test_scan_equals_the_reference_over_the_corpus(dev, corpus, k, nmax):
    for i, batch in enumerate(corpus(k, nmax)):
        _run_batch(dev, batch, GREEDY, 1000 * k + 10 * nmax + i)


def test_scan_equals_the_reference_with_sampled_draws(dev, corpus):
    _run_batch(dev, corpus(3, 4)[0], SAMPLED, 5)


def test_token_ids_at_the_top_of_a_vocabulary_of_262144(dev):
    vocab = 262144
    batch = sc.top_of_vocab(3, 4, vocab)
    d = _run_batch(dev, batch, GREEDY, 9, vocab=vocab, ld=vocab)
    assert int(d["ids"].max()) >= vocab - sc.VOCAB and int(d["hist"].max()) >= vocab - sc.VOCAB + sc.FILL0


# ---- rows that grow across a multiple of 256 with their match in the last positions: a period of five, three periods long at first,
# behind filler that matches nothing -- a scan that missed the last positions would find no match at all

GROW_K, GROW_NMAX, GROW_CALLS, GROW_START = 3, 4, 8, (250, 506, 1018)
PERIOD = [1, 2, 3, 4, 5]


def _grow_initial():
    st = spec_ref.new_state(5, GROW_K, sc.TABLE_STRIDE, sc.HIST_STRIDE, sc.BLOCK_SIZE)
    st["block_table"][:] = np.random.default_rng(3).integers(0, 4096, st["block_table"].shape)
    st["hist"][:] = sc.IDLE
    for r, n in zip((1, 2, 3), GROW_START):  # rows 0 and 4 stay idle
        history = [PERIOD[i % 5] if i >= n - 15 else sc.FILL0 + i % sc.FILL_N for i in range(n)]
        spec_ref.seat(st, r, history, st["block_table"][r].copy(), 1000, GROW_NMAX)
    return st


def _grow_draws(st):
    """every draft comes true and the last draw goes on with the period"""
    draws = np.full((5, GROW_K + 1), sc.JUNK, np.int64)
    for r in (1, 2, 3):
        n = int(st["hist_len"][r])
        draws[r] = [PERIOD[(n + j) % 5] for j in range(GROW_K + 1)]
        assert st["ids"][r, 1:].tolist() == draws[r, :GROW_K].tolist()
    return draws


def test_growing_rows_cross_256_eagerly_and_from_one_graph(dev):
    from qqq_amd import ops

    g = GROW_K + 1
    gen = torch.Generator(device=dev).manual_seed(11)
    par = _params(5, g, GREEDY, gen, dev)
    st = _grow_initial()
    first = spec_ref.copy_state(st)
    d = _to_dev(st, dev)
    bufs, after = [], []
    for i in range(GROW_CALLS):
        draws = _grow_draws(st)
        bufs.append(_logits(draws, sc.VOCAB, LD, gen, dev))
        logits = bufs[i][:, :sc.VOCAB]
        toks = _tokens(ops, logits, par, d["tick"], g)
        assert np.array_equal(toks, draws), i
        _call(ops, logits, par, d, sc.BLOCK_SIZE, GROW_NMAX)
        torch.cuda.synchronize()
        spec_ref.advance(st, toks.tolist(), GROW_NMAX)
        for f in spec_ref.FIELDS:
            assert np.array_equal(d[f].cpu().numpy(), st[f]), (i, f, d[f][1:4].tolist()[-8:], st[f][1:4].tolist()[-8:])
        after.append({f: d[f].clone() for f in spec_ref.FIELDS})
    grown = [n + GROW_CALLS * g for n in GROW_START]
    assert st["hist_len"][1:4].tolist() == grown and st["n_acc"][1:4].tolist() == [GROW_CALLS * GROW_K] * 3
    assert all(n // 256 < m // 256 for n, m in zip(GROW_START, grown))  # every row crossed a multiple of 256
    # the same eight calls from one captured graph, the state and the logits refilled in place
    d = _to_dev(first, dev)
    buf = torch.zeros_like(bufs[0])
    logits = buf[:, :sc.VOCAB]
    buf.copy_(bufs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call(ops, logits, par, d, sc.BLOCK_SIZE, GROW_NMAX)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _call(ops, logits, par, d, sc.BLOCK_SIZE, GROW_NMAX)
    torch.cuda.current_stream().wait_stream(side)
    fresh = _to_dev(first, dev)
    for f in spec_ref.FIELDS:
        d[f].copy_(fresh[f])
    for i in range(GROW_CALLS):
        buf.copy_(bufs[i])
        graph.replay()
        torch.cuda.synchronize()
        for f in spec_ref.FIELDS:
            assert torch.equal(d[f], after[i][f]), (i, f)
