"""ops.topk_logprobs and ops.topk_logprobs_step on the GPU against tests/logprobs_ref.py (float64 numpy): ids and ranks exactly, values
within tests/score_ref.py's tolerance (the bound tests/test_gpu_score.py derives: the values are the scoring kernel's), and bit for bit
against ops.token_logprobs, the on-device oracle.  Ties at the cut, the special values, placement, graph replay, and the step entry on a
hand-made state.

The vocabularies: 40 is under one vector per lane and no multiple of 8; 1027 has a tail; 24581 exceeds one pass of the unrolled walk
(2 x 1024 lanes x 8 tokens) and has a tail; 262144 is the limit (one row).  Every matrix has ld > vocab with NaN and 6e4 in the padding."""
import functools

import numpy as np
import pytest
import torch

import logprobs_ref
from score_ref import tolerance

pytestmark = pytest.mark.gpu

VOCABS = [(40, 48, 3), (1027, 1040, 3), (24581, 24592, 3), (262144, 262152, 1)]  # (vocab, ld, rows)
KS = (0, 1, 5, 32)
SCALES = (1.0, 6.0, 0.5)


def _padded(logits: np.ndarray, ld: int, dev):
    """the rows as a [rows, vocab] view of an fp16 [rows, ld] device matrix whose padding columns hold NaN and 6e4 in turn"""
    rows, vocab = logits.shape
    buf = torch.full((rows, ld), float("nan"), dtype=torch.float16, device=dev)
    buf[:, vocab + 1::2] = 6e4
    buf[:, :vocab] = torch.from_numpy(logits).to(dev)
    return buf[:, :vocab]


def _run(x, tokens, k):
    from qqq_amd import ops

    t = None if tokens is None else torch.as_tensor(np.asarray(tokens, dtype=np.int64)).to(x.device)
    lp, rk, ids, top = ops.topk_logprobs(x, t, k)
    torch.cuda.synchronize()
    rows = x.shape[0]
    if t is None:
        assert lp is None and rk is None
    else:
        assert lp.dtype == torch.float32 and lp.shape == (rows,) and rk.dtype == torch.int32 and rk.shape == (rows,)
    if k == 0:
        assert ids is None and top is None
    else:
        assert ids.dtype == torch.int32 and ids.shape == (rows, k) and top.dtype == torch.float32 and top.shape == (rows, k)
    return tuple(None if a is None else a.cpu().numpy() for a in (lp, rk, ids, top))


def _close(got, ref, what):
    """finite reference values within the scorer's bound; NaN, -inf and 0.0-by-definition exactly"""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref)), (what, got, ref)
    assert np.isfinite(got[fin]).all(), (what, got, ref)
    if fin.any():
        err = np.abs(got[fin] - ref[fin])
        print(f"{what}: max |got - ref| = {err.max():.3e}, max share of the bound = {(err / tolerance(ref[fin])).max():.3f}")
        assert (err <= tolerance(ref[fin])).all(), (what, got, ref)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _against_scorer(x, tokens, got):
    """the existing kernel as the oracle: logprob and every top-k value bit for bit, entry 0 its argmax"""
    from qqq_amd import ops

    lp, rk, ids, top = got
    dev = x.device
    if lp is not None:
        want, am = ops.token_logprobs(x, torch.as_tensor(np.asarray(tokens, dtype=np.int64)).to(dev))
        assert np.array_equal(_bits(lp), _bits(want.cpu().numpy()))
    if ids is not None:
        for i in range(ids.shape[1]):
            want, am = ops.token_logprobs(x, torch.from_numpy(ids[:, i].astype(np.int64)).to(dev))
            assert np.array_equal(_bits(top[:, i]), _bits(want.cpu().numpy())), i
            if i == 0:
                assert am.cpu().numpy().tolist() == ids[:, 0].tolist()


def _check(x, l, tokens, k, what):
    got = _run(x, tokens, k)
    ref = logprobs_ref.topk_logprobs(l, tokens, k)
    if tokens is not None:
        _close(got[0], ref[0], what + " logprob")
        assert got[1].tolist() == ref[1].tolist(), (what, got[1], ref[1])
    if k:
        assert got[2].tolist() == ref[2].tolist(), (what, got[2], ref[2])
        _close(got[3], ref[3], what + " top")
    _against_scorer(x, tokens, got)
    return got


@functools.lru_cache(maxsize=None)
def _case(vocab, rows):
    """random rows (fp16 values repeat: at 24581 tokens nearly every value has ties), their tokens, and the reference at k = 32: once"""
    rng = np.random.default_rng(vocab)
    l = rng.standard_normal((rows, vocab))
    for r in range(rows):
        l[r] *= SCALES[r % len(SCALES)]
    l = l.astype(np.float16)
    tokens = rng.integers(0, vocab, rows)
    tokens[0] = int(l[0].astype(np.float64).argmax())
    ref = logprobs_ref.topk_logprobs(l, tokens, 32)
    return l, tokens, ref


# ---- 1. values, ids and ranks

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("vocab,ld,rows", VOCABS)
def test_against_the_reference_and_the_scorer(dev, vocab, ld, rows, k):
    l, tokens, ref = _case(vocab, rows)
    x = _padded(l, ld, dev)
    got = _run(x, tokens, k)
    _close(got[0], ref[0], f"vocab {vocab} k {k} logprob")
    assert got[1].tolist() == ref[1].tolist() and got[1][0] == 1
    if k:
        assert got[2].tolist() == ref[2][:, :k].tolist()
        _close(got[3], ref[3][:, :k], f"vocab {vocab} k {k} top")
        only = _run(x, None, k)  # without a token: the same top-k
        assert np.array_equal(only[2], got[2]) and np.array_equal(_bits(only[3]), _bits(got[3]))
    _against_scorer(x, tokens, got)


# ---- 2. ties

@pytest.mark.parametrize("k", [1, 5, 32])
def test_an_all_equal_row_gives_the_lowest_indices(dev, k):
    vocab = 1027
    l = np.full((2, vocab), 1.5, np.float16)
    l[1] = -3.0
    got = _check(_padded(l, 1032, dev), l, [5, 1026], k, f"all equal k {k}")
    assert got[2].tolist() == [list(range(k))] * 2 and got[1].tolist() == [1, 1]


def _plateau_row(vocab, distinct, plateau, seed):
    """`distinct` distinct values on top, then `plateau` equal values scattered over the row, the rest below"""
    rng = np.random.default_rng(seed)
    row = rng.uniform(-6.0, 1.0, vocab).astype(np.float16)
    perm = rng.permutation(vocab)
    row[perm[:distinct]] = (10.0 + 0.5 * np.arange(distinct)).astype(np.float16)
    row[perm[distinct:distinct + plateau]] = 3.0
    return row, np.sort(perm[distinct:distinct + plateau])


@pytest.mark.parametrize("k", [5, 32])
def test_the_cut_falls_inside_a_plateau_that_spans_many_waves(dev, k):
    vocab = 24581
    row, members = _plateau_row(vocab, k - 2, 5000, k)
    assert members[1] // (8 * 193) != members[-1] // (8 * 193)  # the tie set is not one wave's part of the row
    l = row[None]
    got = _check(_padded(l, 24592, dev), l, [int(members[2])], k, f"plateau at the cut k {k}")
    assert got[2][0, k - 2:].tolist() == members[:2].tolist()  # the two lowest indices of the plateau
    assert got[1][0] == k - 1                                  # the token is a member outside the top-k: k - 2 values above it


def test_a_plateau_wholly_below_the_cut(dev):
    vocab, k = 24581, 5
    row, members = _plateau_row(vocab, 8, 5000, 77)
    l = row[None]
    got = _check(_padded(l, 24592, dev), l, [int(members[-1])], k, "plateau below the cut")
    assert not set(got[2][0].tolist()) & set(members.tolist()) and got[1][0] == 9


# ---- 3. special values

def test_special_values(dev):
    vocab, ld, k = 1027, 1032, 5
    rng = np.random.default_rng(9)
    base = rng.uniform(-4.0, -1.0, vocab).astype(np.float16)
    rows, tokens = [], []

    def add(row, t):
        rows.append(row.astype(np.float16))
        tokens.append(t)
        return len(rows) - 1

    dead = np.full(vocab, -np.inf, np.float16)
    dead[::3] = np.nan
    r_dead = add(dead, 7)                                   # only NaN and -inf
    few = dead.copy()
    few[[900, 13, 400]] = [1.0, 2.0, 1.0]
    r_few = add(few, 1)                                     # three finite logits, k = 5; the token's logit is -inf
    inf = base.copy()
    inf[[50, 700]] = np.inf
    r_inf = add(inf, 700)                                   # +inf: its tie group shares the mass
    r_inf_fin = add(inf, 3)                                 # ... and a finite token has none
    zero = base.copy()
    zero[2], zero[7] = -0.0, 0.0
    r_zero = add(zero, 7)                                   # -0 == +0: index order, rank 1 for both
    r_neg = add(base, -1)                                   # ignored
    r_big = add(base, vocab)                                # a bad token
    l = np.stack(rows)
    got = _check(_padded(l, ld, dev), l, tokens, k, "special values")
    lp, rk, ids, top = got
    assert np.isnan(lp[r_dead]) and rk[r_dead] == 1 and ids[r_dead].tolist() == [0, 1, 2, 3, 4] and np.isnan(top[r_dead]).all()
    assert ids[r_few].tolist() == [13, 400, 900, 0, 1] and np.isneginf(top[r_few, 3:]).all() and np.isfinite(top[r_few, :3]).all()
    assert np.isneginf(lp[r_few]) and rk[r_few] == 4
    assert ids[r_inf, :2].tolist() == [50, 700] and abs(float(lp[r_inf]) + np.log(2.0)) < 1e-6 and rk[r_inf] == 1
    assert np.isneginf(lp[r_inf_fin]) and np.isneginf(top[r_inf, 2:]).all()
    assert ids[r_zero, :2].tolist() == [2, 7] and rk[r_zero] == 1 and _bits(top[r_zero, :1]) == _bits(top[r_zero, 1:2])
    assert float(lp[r_neg]) == 0.0 and rk[r_neg] == 0 and np.isnan(lp[r_big]) and rk[r_big] == 0
    assert ids[r_neg].tolist() == ids[r_big].tolist()  # the top-k part does not depend on the token


# ---- 4. the same row, the same bits

def test_a_row_gives_the_same_bits_wherever_it_sits(dev):
    vocab, k = 24581, 32
    l, tokens, _ = _case(vocab, 3)
    row, t = l[1], int(tokens[1])
    other = np.random.default_rng(2).standard_normal((5, vocab)).astype(np.float16)
    other[3] = row
    a = _run(_padded(row[None], 24592, dev), [t], k)
    b = _run(_padded(other, 24584 + 64, dev), [0, 1, 2, t, 4], k)
    c = _run(torch.from_numpy(row[None].copy()).to(dev), [t], k)  # an unpadded view: the op copies it into padded rows
    for got, r in ((b, 3), (c, 0)):
        assert _bits(got[0][r:r + 1]) == _bits(a[0][:1]) and got[1][r] == a[1][0]
        assert np.array_equal(got[2][r], a[2][0]) and np.array_equal(_bits(got[3][r]), _bits(a[3][0]))


def test_hipgraph_replays_with_everything_updated_in_place(dev):
    from qqq_amd import ops

    rows, vocab, k = 4, 4099, 5
    g = torch.Generator(device=dev).manual_seed(1)
    buf = torch.zeros((rows, vocab + 5), dtype=torch.float16, device=dev)
    logits = buf[:, :vocab]
    tokens = torch.zeros(rows, dtype=torch.int64, device=dev)

    def fill(i):
        logits.copy_((3.0 * torch.randn((rows, vocab), generator=g, device=dev)).half())
        tokens.copy_(torch.randint(0, vocab, (rows,), generator=g, device=dev))
        tokens[i % rows] = -1

    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.topk_logprobs(logits, tokens, k)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = ops.topk_logprobs(logits, tokens, k)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for i in range(1, 4):
        fill(i)
        graph.replay()
        torch.cuda.synchronize()
        want = ops.topk_logprobs(logits, tokens, k)
        torch.cuda.synchronize()
        for a, b in zip(out, want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        ref = logprobs_ref.topk_logprobs(logits.cpu().numpy(), tokens.cpu().numpy(), k)
        assert out[2].cpu().numpy().tolist() == ref[2].tolist() and out[1].cpu().numpy().tolist() == ref[1].tolist()
        _close(out[0].cpu().numpy(), ref[0], f"replay {i}")
        assert float(out[0][i % rows]) == 0.0
        seen.append(out[2].tolist())
    assert seen[0] != seen[1] and seen[1] != seen[2]  # the replays read the new contents


# ---- 5. the step entry on a hand-made state

@pytest.mark.parametrize("k", [0, 5])
def test_step_entry_writes_one_record_where_a_token_waits(dev, k):
    from qqq_amd import ops

    vocab, rows, cap, stride = 1027, 6, 4, 6
    l, _, _ = _case(vocab, 3)
    l = np.concatenate([l, l[::-1]])
    x = _padded(l, 1040, dev)
    rng = np.random.default_rng(4)
    out = torch.from_numpy(rng.integers(0, vocab, (rows, stride))).to(dev)
    # row 0: first token; 1: caught up; 2: third token; 3: no room (n_rec == cap); 4: two tokens behind; 5: idle, never used
    n_out = torch.tensor([1, 2, 3, 5, 3, 0], dtype=torch.int32, device=dev)
    n_rec = torch.tensor([0, 2, 2, 4, 1, 0], dtype=torch.int32, device=dev)
    writes = {0: 0, 2: 2, 4: 1}
    lp = torch.full((rows, cap), 7.0, device=dev)
    rk = torch.full((rows, cap), -7, dtype=torch.int32, device=dev)
    ids = torch.full((rows, cap, k), -7, dtype=torch.int32, device=dev) if k else None
    top = torch.full((rows, cap, k), 7.0, device=dev) if k else None
    before = [None if a is None else a.clone() for a in (lp, rk, ids, top)]
    ops.topk_logprobs_step(x, out, n_out, n_rec, lp, rk, ids, top)
    torch.cuda.synchronize()
    assert n_rec.tolist() == [1, 2, 3, 4, 2, 0]
    toks = torch.tensor([int(out[r, writes.get(r, 0)]) for r in range(rows)], dtype=torch.int64, device=dev)
    want = ops.topk_logprobs(x, toks, k)
    for r in range(rows):
        for got, old, new in zip((lp, rk, ids, top), before, want):
            if got is None:
                continue
            for a in range(cap):
                exp = new[r] if writes.get(r) == a else old[r, a]
                assert torch.equal(got[r, a].reshape(-1).view(torch.int32), exp.reshape(-1).view(torch.int32)), (r, a)
    # a second call without a new token: row 4 is still one behind and writes record 2, nothing else moves
    state = [None if a is None else a.clone() for a in (lp, rk, ids, top)]
    ops.topk_logprobs_step(x, out, n_out, n_rec, lp, rk, ids, top)
    torch.cuda.synchronize()
    assert n_rec.tolist() == [1, 2, 3, 4, 3, 0]
    ops.topk_logprobs_step(x, out, n_out, n_rec, lp, rk, ids, top)  # ... and now nobody owes a record
    torch.cuda.synchronize()
    assert n_rec.tolist() == [1, 2, 3, 4, 3, 0]
    for got, old in zip((lp, rk, ids, top), state):
        if got is None:
            continue
        keep = torch.ones((rows, cap), dtype=torch.bool, device=dev)
        keep[4, 2] = False
        assert torch.equal(got[keep].view(torch.int32), old[keep].view(torch.int32))
    assert int(rk[4, 2]) == int(ops.topk_logprobs(x[4:5], out[4:5, 2].contiguous(), 0)[1][0])
