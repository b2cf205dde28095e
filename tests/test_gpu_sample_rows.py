"""ops.sample_tokens on the rows of tests/sample_rows.py, exactly: the surviving set and the token of every u of a grid on sparse rows whose
weight lies at the first and last token of waves, draw steps and histogram passes; the fixed-point sums at their bound on flat rows; cuts
between plateaus of one level-1 bin; and per-row parameters in one launch and from a captured graph.  tests/test_sample_rows_cpu.py proves
the conditions these tests rely on without a GPU."""
import numpy as np
import pytest
import torch

import sample_rows as S
from sample_ref import sample_row, sample_rows
from test_gpu_sample import EPS, _run

pytestmark = pytest.mark.gpu

CASE_NAMES = ("none", "k", "p", "k+p", "k60", "k+plow")


def _tiled(l, n, dev):
    """n copies of the row as a [n, vocab] view of a matrix with ld = vocab rounded up to 8, whose padding columns hold 65504"""
    vocab = l.shape[0]
    buf = torch.full((n, (vocab + 7) // 8 * 8), 65504.0, dtype=torch.float16, device=dev)
    buf[:, :vocab] = torch.from_numpy(np.array(l)).to(dev)
    return buf[:, :vocab]


def _dyadic(n=256):
    return (np.arange(n) / n).astype(np.float32)


ALMOST_ONE = np.nextafter(np.float32(1), np.float32(0))


def _between(n=256):
    """one u inside every 1 / n, off the dyadic grid: where a row repeats with a period that divides vocab / n, a dyadic u always draws
    the first token of a period -- the same lane, the same element, the same plateau"""
    return np.minimum((np.arange(n) + np.random.default_rng(n).random(n)) / n, ALMOST_ONE).astype(np.float32)


def _exact_tokens(w, u):
    """the draw of include/qqq_amd_sample.h in integers, for fixed-point weights w (int64; 0 where a token is cut; their sum at most 2^62
    and exact as an f64): the lowest j with c_j > u * W2, that product in f64 and rounded down"""
    c = np.cumsum(w)
    W2 = int(c[-1])
    assert int(float(W2)) == W2 and W2 <= 2 ** 62
    target = np.floor(np.minimum(u, ALMOST_ONE).astype(np.float64) * np.float64(W2)).astype(np.int64)
    return np.searchsorted(c, np.minimum(target, W2 - 1), side="right")


# ---- a. sparse rows: the surviving set and the token, exact

@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("T", S.TS)
@pytest.mark.parametrize("vocab", S.VOCABS)
def test_sparse_rows_exact_set_and_token_through_a_u_grid(dev, vocab, T, name):
    l, pos = S.sparse_row(vocab)
    (k, p), = [(k, p) for t, k, p, nm in S.cases(vocab) if t == T and nm == name]
    ref = S.sparse_ref(vocab, T, k, p)
    n = S.grid_n(vocab)
    u = S.u_grid(n)
    got = _run(_tiled(l, n, dev), T, k, float(p), u)
    assert ((got >= 0) & (got < vocab)).all()
    assert ref.survive[got].all(), ("outside the surviving set", sorted(set(got[~ref.survive[got]].tolist()))[:10])
    likely = pos[ref.survive[pos] & (ref.prob[pos] > 2.0 / n)]
    assert np.isin(likely, got).all(), ("never drawn", likely[~np.isin(likely, got)])
    assert (np.diff(got) >= 0).all()
    clear, want = ref.clear(u), ref.tokens(u)
    assert clear.mean() >= 0.98
    bad = np.nonzero(clear & (got != want))[0]
    e = np.concatenate([[0.0], ref.edges])
    print(f"vocab {vocab} {name} T {T}: compared {int(clear.sum())} of {n} points, {int((got != want).sum())} differ within EPS of an edge")
    assert bad.size == 0, [(float(u[i]), int(got[i]), int(want[i]), f"{np.abs(e - float(u[i])).min():.2e} from an edge") for i in bad[:8]]
    counts = np.bincount(got, minlength=vocab)
    assert np.abs(counts - n * ref.prob).max() <= 2.0


# ---- b. flat rows: 2^18 terms of 2^44

@pytest.mark.parametrize("value", [0.0, -3.5])
@pytest.mark.parametrize("vocab", [262144, 16411])
def test_flat_rows_draw_floor_u_vocab(dev, vocab, value):
    x = _tiled(S.flat_row(vocab, value), 256, dev)
    u, ub = _dyadic(), _between()
    want = [i * vocab // 256 for i in range(256)]
    wantb = _exact_tokens(np.full(vocab, 2 ** 44, np.int64), ub)
    assert np.unique(wantb % 8).size == 8 and np.unique(wantb // 8 % 64).size > 32  # every element of a vector, most lanes
    for T in (1.0, 0.7):
        for k, p in ((0, 1.0), (5, 1.0), (0, 0.3), (5, 0.3), (0, 0.0)):  # the whole row is the maximum's tie group: both cuts keep it whole
            assert _run(x, T, k, p, u).tolist() == want, (T, k, p)
            assert _run(x, T, k, p, ub).tolist() == wantb.tolist(), (T, k, p)
            assert _run(x[:1], T, k, p, [ALMOST_ONE]).tolist() == [vocab - 1], (T, k, p)


# ---- c. plateaus: cuts inside one level-1 bin

def _mid_gap_p(l, T, k, group):
    """p with 1 - p in the middle of tie group `group`'s share of the kept mass (groups from the least probable up): that group and the
    ones above it survive.  The cut is >= 1e-3 from both edges."""
    p, gap = S._tie_group_gaps(l, T, k)[group]
    assert gap >= 2e-3, (T, k, group, gap)
    return float(p)


def _beside_edge_p(l, T, k, group, off):
    """p with 1 - p at `off` (+-2e-3) from the lower edge of tie group `group`: twice the 1e-3 that a cut keeps from every edge here"""
    e = S.tie_group_edges(l, T, k)
    x = e[group] + off
    assert np.abs(e - x).min() >= 1.9e-3
    return float(np.float32(1.0 - x))


@pytest.mark.parametrize("T", ["pow2", 1.0])
@pytest.mark.parametrize("abc", [S.SAME_BYTE, S.OTHER_BYTE, S.ONE_BIN], ids=["same_high_byte", "other_high_byte", "one_bin"])
@pytest.mark.parametrize("vocab", [16411, 262144])
def test_two_level_rows_cut_between_plateaus(dev, vocab, abc, T):
    exact = T == "pow2"  # the temperature at which the kernel's weights of these plateaus are powers of two
    T = S.T_POW2[abc] if exact else T
    l = S.two_level_row(vocab, abc)
    v = l.astype(np.float64)
    is_a, is_b = v == abc[0], v == abc[1]
    m = int(is_a.sum())
    assert m == (vocab + 1) // 2
    x = _tiled(l, 256, dev)
    u = _dyadic()
    plateaus = {"a": is_a, "ab": is_a | is_b, "abc": np.ones(vocab, bool)}
    cases = [(3, 1.0, "a"), (m + 1, 1.0, "ab"), (0, 1.0, "abc"),
             (0, _mid_gap_p(l, T, 0, 2), "a"), (0, _mid_gap_p(l, T, 0, 1), "ab"), (0, _mid_gap_p(l, T, 0, 0), "abc"),
             (m + 1, _mid_gap_p(l, T, m + 1, 1), "a"),   # top-p cuts above top-k, in its level-1 bin where a and b share a high byte
             (m + 1, _mid_gap_p(l, T, m + 1, 0), "ab"),  # top-p's cut inside the top-k threshold's own tie group
             (3, _mid_gap_p(l, T, 3, 0), "a"),
             # top-p beside the edge between b and a, under a top-k that drops c: c's mass counted into W (left in top-k's level-2
             # masses where c shares b's bin, in the level-1 masses where it does not) would move the cut across that edge
             (m + 1, _beside_edge_p(l, T, m + 1, 1, 2e-3), "a"), (m + 1, _beside_edge_p(l, T, m + 1, 1, -2e-3), "ab")]
    # the kernel's fixed-point weights where log2 e / T is a power of two: 2^44 times an exact power of two
    scale = S.POW2_SCALE[abc]
    fixed = np.array([2 ** (44 + int(round(scale * (t - abc[0])))) for t in abc], np.int64)[np.searchsorted(-np.array(abc), -v)]
    for k, p, keeps in cases:
        ref = sample_row(l, T, k, p, 0.0)
        assert (ref["survive"] == plateaus[keeps]).all(), (k, p, keeps)
        surv = np.nonzero(ref["survive"])[0]
        assert _run(x[:1], T, k, p, [ALMOST_ONE])[0] == surv[-1], (k, p, keeps)
        for dyadic, u in ((True, _dyadic()), (False, _between())):
            got = _run(x, T, k, p, u)
            assert ref["survive"][got].all() and (np.diff(got) >= 0).all(), (k, p, keeps, dyadic)
            if keeps == "a":  # every survivor weighs 2^44, whatever T: for a dyadic u the floor(u m)-th survivor
                if dyadic:
                    assert got.tolist() == [int(surv[i * m // 256]) for i in range(256)], (k, p, keeps)
                assert got.tolist() == _exact_tokens(np.where(is_a, 2 ** 44, 0), u).tolist(), (k, p, keeps, dyadic)
            elif exact:
                assert got.tolist() == _exact_tokens(np.where(ref["survive"], fixed, 0), u).tolist(), (k, p, keeps, dyadic)
            else:
                # the tokens lie closer than EPS to each other here (1 / vocab of the mass each), so no point is clear of every edge:
                # the window of test_large_rows_within_the_derived_tolerance on the drawn token's own interval
                cc, W2 = ref["c"], ref["W2"]
                lo = np.where(got > 0, cc[np.maximum(got - 1, 0)], 0.0)
                xs = u.astype(np.float64) * W2
                assert ((lo - EPS * W2 <= xs) & (xs <= cc[got] + EPS * W2)).all(), (k, p, keeps, dyadic)
            if keeps != "a" and not dyadic:
                assert is_b[got].any(), (k, p, keeps)  # this grid does see the second plateau


# ---- d. per-row parameters in one launch, and from a captured graph

def _mixed(shift):
    vocab, rows = 8200, 24
    l = np.empty((rows, vocab), np.float16)
    for r in range(rows):
        j = (r + shift) % rows
        l[r] = (S.sparse_row(vocab, seed=j // 3 % 2)[0], S.flat_row(vocab, (0.0, -3.5, 7.0)[j // 3 % 3]),
                S.two_level_row(vocab, (S.SAME_BYTE, S.OTHER_BYTE, S.ONE_BIN)[j // 3 % 3]))[j % 3]
    rng = np.random.default_rng(shift)
    cyc = lambda vals, step: np.array([vals[(r * step + shift) % len(vals)] for r in range(rows)])  # noqa: E731
    T = cyc([1.0, 0.0, 0.5, 2.0, S.T_POW2[S.SAME_BYTE], -1.0, 1.0], 1).astype(np.float32)
    k = cyc([0, S.k_tie(), 1, 60, 3, 4101, 0], 5).astype(np.int32)
    p = cyc([1.0, 0.5, 0.9, 0.3, 0.0], 7).astype(np.float32)
    return l, T, k, p, rng.random(rows).astype(np.float32)


def _alone(x, T, k, p, u):
    return [int(_run(x[r:r + 1], [T[r]], [k[r]], [p[r]], [u[r]])[0]) for r in range(x.shape[0])]


def test_rows_with_their_own_parameters_give_what_they_give_alone(dev):
    l, T, k, p, u = _mixed(0)
    assert (T <= 0).sum() >= 4 and (k == 1).sum() >= 2
    x = _tiled(l[0], l.shape[0], dev)
    x.copy_(torch.from_numpy(l).to(dev))
    got = _run(x, T, k, p, u).tolist()
    assert got == _alone(x, T, k, p, u)
    ref = sample_rows(l, T, k, p, u)
    assert all(o["token"] == t if o["greedy"] else o["survive"][t] for o, t in zip(ref, got))
    assert len(set(got)) > 8


def test_hipgraph_replays_mixed_rows_rewritten_in_place(dev):
    from qqq_amd import ops

    l, T, k, p, u = _mixed(0)
    rows = l.shape[0]
    x = _tiled(l[0], rows, dev)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    Tt, kt, pt, ut = t(T), t(k), t(p), t(u)
    x.copy_(t(l))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.sample_tokens(x, Tt, kt, pt, ut)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = ops.sample_tokens(x, Tt, kt, pt, ut)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for shift in (1, 2, 5):
        l, T, k, p, u = _mixed(shift)
        for dst, src in ((x, l), (Tt, T), (kt, k), (pt, p), (ut, u)):
            dst.copy_(t(src))
        graph.replay()
        torch.cuda.synchronize()
        got = out.tolist()
        assert got == _alone(x, T, k, p, u), shift
        seen.append(got)
    assert seen[0] != seen[1] != seen[2]
