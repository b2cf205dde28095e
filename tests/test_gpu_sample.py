"""ops.sample_tokens on the GPU against tests/sample_ref.py (float64 numpy): greedy rows exactly, the surviving set exactly through a grid of
uniform variates, large rows within a derived tolerance, the special values, and replay from a captured graph."""
import numpy as np
import pytest
import torch

from sample_ref import sample_row, sample_rows

pytestmark = pytest.mark.gpu


def _padded(logits: np.ndarray, ld: int, dev, fill=65504.0):
    """the rows as a [rows, vocab] view of an fp16 [rows, ld] device matrix whose padding columns hold `fill`"""
    rows, vocab = logits.shape
    buf = torch.full((rows, ld), fill, dtype=torch.float16, device=dev)
    buf[:, :vocab] = torch.from_numpy(logits).to(dev)
    return buf[:, :vocab]


def _run(logits, T, k, p, u):
    from qqq_amd import ops

    dev = logits.device
    t = lambda v, dt: v if not isinstance(v, (np.ndarray, list)) else torch.tensor(np.asarray(v), dtype=dt, device=dev)  # noqa: E731
    out = ops.sample_tokens(logits, t(T, torch.float32), t(k, torch.int32), t(p, torch.float32),
                            torch.tensor(np.asarray(u, dtype=np.float32), device=dev))
    torch.cuda.synchronize()
    assert out.dtype == torch.int64 and out.shape == (logits.shape[0],)
    return out.cpu().numpy()


# ---- 1. greedy rows, exact

@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("vocab,ld", [(1, 8), (7, 8), (63, 64), (64, 64), (65, 72), (1001, 1008), (32000, 32000), (65537, 65544),
                                      (151936, 151936)])
def test_greedy_is_the_lowest_index_of_the_maximum(dev, vocab, ld, rows):
    rng = np.random.default_rng(vocab * 7 + rows)
    for place in ("first", "last", "dup"):
        if place == "dup" and vocab < 2:
            continue
        l = rng.standard_normal((rows, vocab)).astype(np.float16)
        for r in range(rows):
            at = {"first": [0], "last": [vocab - 1]}.get(place) or sorted(rng.choice(vocab, size=min(3, vocab), replace=False).tolist())
            l[r, at] = 30.0
        x = _padded(l, ld, dev)  # padding columns hold 65504: they must not win
        want = l.astype(np.float64).argmax(axis=1)
        zeros, ones = np.zeros(rows, np.float32), np.ones(rows, np.float32)
        u = rng.random(rows).astype(np.float32)
        for T, k, p, uu in ((zeros, 0, ones, u), (ones * -1, 0, ones, u), (ones, 1, ones, u), (ones, 0, zeros, zeros),
                            (ones, 0, -ones, zeros), (ones, 40, zeros, zeros)):
            got = _run(x, T, np.full(rows, k, np.int32), p, uu)
            ref = [o["token"] for o in sample_rows(l, T, np.full(rows, k), p, uu)]
            assert got.tolist() == ref == want.tolist(), (place, T[0], k, p[0])


# ---- 2. the surviving set, exact, through a grid of u

def _grid_row():
    # multiples of 0.25 in [0, 3], both ends present, skewed towards 0: few tokens share the top, so that even at T = 0.5 and without a
    # cut the least probable token (e^-6 of the most probable) keeps more than 2 / 4096 of the mass (asserted in the test)
    rng = np.random.default_rng(24)
    lv = np.minimum((rng.random(50) ** 2 * 13).astype(int), 12)
    lv[rng.choice(50, 2, replace=False)] = [0, 12]
    l = (lv * 0.25).astype(np.float16)
    srt = np.sort(l.astype(np.float64))[::-1]
    k = next(k for k in range(8, 40) if srt[k - 1] == srt[k])  # a tie at the k-th largest value
    return l, k


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("use_k,use_p", [(True, False), (False, True), (True, True), (False, False)])
def test_surviving_set_and_frequencies_through_a_u_grid(dev, use_k, use_p, T):
    n = 4096
    l, k = _grid_row()
    k = k if use_k else 0
    p = 0.8 if use_p else 1.0
    u = ((np.arange(n) + 0.5) / n).astype(np.float32)
    ref = sample_row(l, T, k, p, 0.0)
    surv = np.nonzero(ref["survive"])[0]
    if use_k:
        assert ref["survive"].sum() > k or use_p  # the tie at the k-th value is kept whole
    if use_p:  # the cut is not within rounding of a tie group's edge
        order = np.argsort(l.astype(np.float64), kind="stable")
        w = np.diff(np.concatenate([[0.0], sample_row(l, T, k, 1.0, 0.0)["c"]]))
        cum = np.cumsum(w[order]) / w.sum()
        assert np.abs(cum - (1.0 - np.float64(np.float32(p)))).min() > 1e-6
    got = _run(torch.from_numpy(np.tile(l, (n, 1))).to(dev), T, k, p, u)
    assert sorted(set(got.tolist())) == surv.tolist()
    assert (np.diff(got) >= 0).all()
    ws = np.diff(np.concatenate([[0.0], ref["c"]]))
    prob = ws / ref["W2"]
    assert prob[surv].min() > 2.0 / n
    counts = np.bincount(got, minlength=50)
    # +-1: a grid against an interval's length; +-1: an edge moved by rounding
    assert np.abs(counts - n * prob).max() <= 2.0, (counts, n * prob)


# ---- 3. large rows, with the derived tolerance

CASES = [dict(T=0.7, k=0, p=None), dict(T=1.0, k=0, p=None), dict(T=1.5, k=0, p=None), dict(T=1.0, k=50, p=None),
         dict(T=1.5, k=50, p="gap"), dict(T=1.0, k=0, p="gap")]
EPS = 1e-4  # f32 exp of an argument up to ~45: <~3e-6 relative; a sum of up to 2^18 non-negative terms: <~4e-5; twice their sum


def _top_p_in_the_widest_gap(l, T, k):
    """p with 1 - p at the midpoint of the widest gap between successive tie-group cumulative masses (from the least probable kept token
    up, as fractions of W) whose lower edge lies in (0.05, 0.7); returns (p, gap)"""
    base = sample_row(l, T, k, 1.0, 0.0)
    w = np.diff(np.concatenate([[0.0], base["c"]]))
    vals, inv = np.unique(l.astype(np.float64), return_inverse=True)
    cum = np.cumsum(np.bincount(inv, weights=w, minlength=vals.size)) / w.sum()
    lo, hi = cum[:-1], cum[1:]
    ok = (lo > 0.05) & (lo < 0.7)
    i = np.argmax(np.where(ok, hi - lo, -1.0))
    return np.float32(1.0 - 0.5 * (lo[i] + hi[i])), float(hi[i] - lo[i])


@pytest.mark.parametrize("vocab", [32000, 128256, 151936])
def test_large_rows_within_the_derived_tolerance(dev, vocab):
    rows = 16
    rng = np.random.default_rng(vocab)
    l = (4.0 * rng.standard_normal((rows, vocab))).astype(np.float16)
    u = rng.random(rows).astype(np.float32)
    T = np.array([CASES[r % len(CASES)]["T"] for r in range(rows)], np.float32)
    k = np.array([CASES[r % len(CASES)]["k"] for r in range(rows)], np.int32)
    p = np.ones(rows, np.float32)
    for r in range(rows):
        if CASES[r % len(CASES)]["p"] == "gap":
            p[r], gap = _top_p_in_the_widest_gap(l[r], T[r], int(k[r]))
            assert gap >= 4e-3, (r, gap)  # before any launch: the cut is far from every tie group's edge
    refs = sample_rows(l, T, k, p, u)
    got = _run(torch.from_numpy(l).to(dev), T, k, p, u)
    for r in range(rows):
        t, ref = int(got[r]), refs[r]
        assert 0 <= t < vocab and ref["survive"][t], (r, t, "not in the surviving set")  # top-k is integer counting: no tolerance
        c, W2 = ref["c"], ref["W2"]
        lo = c[t - 1] if t else 0.0
        x = float(u[r]) * W2
        print(f"vocab {vocab} row {r}: token {t} (ref {ref['token']}), survivors {int(ref['survive'].sum())}, "
              f"(u W2 - c[t-1]) / W2 = {(x - lo) / W2:.3e}, (c[t] - u W2) / W2 = {(c[t] - x) / W2:.3e}")
        assert lo - EPS * W2 <= x <= c[t] + EPS * W2, (r, t, ref["token"])


# ---- 4. edges

def test_edges_of_u_and_single_survivors(dev):
    rng = np.random.default_rng(11)
    vocab = 777
    l = rng.standard_normal((1, vocab)).astype(np.float16)
    x = torch.from_numpy(l).to(dev)
    for T, k, p in ((1.0, 0, 1.0), (0.8, 20, 0.9), (1.3, 0, 0.5)):
        ref = sample_row(l[0], T, k, p, 0.0)
        surv = np.nonzero(ref["survive"])[0]
        assert _run(x, T, k, p, [0.0])[0] == surv[0] == ref["token"]
        assert _run(x, T, k, p, [np.nextafter(np.float32(1), np.float32(0))])[0] in surv
        assert _run(x, T, k, p, [1.5])[0] in surv
        assert _run(x, T, k, p, [-1.0])[0] == surv[0]
        assert _run(x, T, k, p, [float("nan")])[0] == surv[0]
    # a single survivor: one logit far above the rest, whatever u
    l2 = l.copy()
    l2[0, 123] = 60.0
    assert set(_run(torch.from_numpy(np.tile(l2, (8, 1))).to(dev), 1.0, 0, 1.0, np.linspace(0, 0.999, 8)).tolist()) == {123}
    l3 = l.copy()
    l3[0, 500] = 9.0
    assert set(_run(torch.from_numpy(np.tile(l3, (8, 1))).to(dev), 1.0, 5, 1e-3, np.linspace(0, 0.999, 8)).tolist()) == {500}


def test_special_values_stay_in_range(dev):
    vocab, ld = 300, 304
    rng = np.random.default_rng(3)
    base = rng.standard_normal(vocab).astype(np.float16)
    rows = []
    rows.append(np.full(vocab, -np.inf, np.float16))                      # 0: nothing finite -> 0
    rows.append(np.full(vocab, np.nan, np.float16))                       # 1: nothing finite -> 0
    rows.append(np.full(vocab, np.inf, np.float16))                       # 2: nothing finite -> 0
    a = base.copy(); a[[7, 200]] = np.inf; rows.append(a)                 # 3: +inf beside finite values: its tie group
    a = base.copy(); a[::2] = np.nan; a[1] = -np.inf; rows.append(a)      # 4: NaN and -inf have no weight
    a = np.full(vocab, np.nan, np.float16); a[250] = -3.0; rows.append(a)  # 5: one finite logit
    a = np.full(vocab, -np.inf, np.float16); a[[10, 20]] = 0.0; a[20] = -0.0; rows.append(a)  # 6: -0 ties with +0
    l = np.stack(rows)
    x = _padded(l, ld, dev, fill=float("inf"))
    n = l.shape[0]
    for T, k, p in ((1.0, 0, 1.0), (0.0, 0, 1.0), (1.0, 3, 0.7), (float("inf"), 0, 0.9), (1e-30, 2, 0.5), (float("nan"), 0, float("nan")),
                    (1.0, 0, float("nan")), (1.0, -5, -1.0), (1.0, 2 ** 31 - 1, 2.0), (1e30, 4, 1e-30)):
        for u in (0.0, 0.37, 0.999):
            got = _run(x, T, k, p, np.full(n, u, np.float32))
            ref = sample_rows(l, T, k, p, np.full(n, u, np.float32))
            assert ((got >= 0) & (got < vocab)).all(), (T, k, p, u, got)
            assert got[:3].tolist() == [0, 0, 0]
            for r in range(n):
                assert ref[r]["greedy"] or ref[r]["W2"] == 0 or ref[r]["survive"][got[r]], (T, k, p, u, r, got[r])
            if u == 0.0:
                assert got.tolist() == [o["token"] for o in ref], (T, k, p)
    # NaN T is greedy; NaN p keeps the top-k set
    got = _run(x[4:5], float("nan"), 0, 0.5, [0.9])
    assert got[0] == sample_row(l[4], float("nan"), 0, 0.5, 0.9)["token"] == int(np.nanargmax(np.where(np.isnan(l[4].astype(np.float64)), -np.inf, l[4])))
    assert sample_row(l[4], 1.0, 4, float("nan"), 0.0)["survive"].sum() == 4
    seen = set(_run(x[4:5].expand(64, vocab), 1.0, 4, float("nan"), np.linspace(0, 0.999, 64)).tolist())
    assert seen == set(np.nonzero(sample_row(l[4], 1.0, 4, float("nan"), 0.0)["survive"])[0].tolist())


# ---- 5. graph replay

def test_hipgraph_replays_with_everything_updated_in_place(dev):
    from qqq_amd import ops

    rows, vocab = 6, 4099
    g = torch.Generator(device=dev).manual_seed(1)
    buf = torch.zeros((rows, vocab + 5), dtype=torch.float16, device=dev)
    logits = buf[:, :vocab]
    T = torch.ones(rows, device=dev)
    k = torch.zeros(rows, dtype=torch.int32, device=dev)
    p = torch.ones(rows, device=dev)
    u = torch.zeros(rows, device=dev)

    def fill(i):
        logits.copy_((3.0 * torch.randn((rows, vocab), generator=g, device=dev)).half())
        T.copy_(torch.tensor([0.0, 0.7, 1.0, 1.5, 1.0, 2.0], device=dev).roll(i))
        k.copy_(torch.tensor([0, 0, 40, 7, 0, 1], dtype=torch.int32, device=dev).roll(i))
        p.copy_(torch.tensor([1.0, 0.9, 1.0, 0.8, 0.5, 0.95], device=dev).roll(2 * i))
        u.copy_(torch.rand(rows, generator=g, device=dev))

    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.sample_tokens(logits, T, k, p, u)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = ops.sample_tokens(logits, T, k, p, u)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for i in range(1, 4):
        fill(i)
        graph.replay()
        torch.cuda.synchronize()
        want = ops.sample_tokens(logits, T, k, p, u)
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        ref = sample_rows(logits.cpu().numpy(), T.cpu().numpy(), k.cpu().numpy(), p.cpu().numpy(), u.cpu().numpy())
        assert all(o["greedy"] and o["token"] == t or o["survive"][t] for o, t in zip(ref, out.tolist()))
        seen.append(out.tolist())
    assert seen[0] != seen[1] or seen[1] != seen[2]  # the replays read the new contents
