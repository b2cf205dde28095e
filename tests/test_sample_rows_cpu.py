"""tests/sample_rows.py held to its conditions by tests/sample_ref.py alone, without a GPU: what tests/test_gpu_sample_rows.py relies on
before any launch -- where the hot tokens lie, that the filler has no mass, that few grid points lie near an edge, and which branch of the
kernel's top-p each case takes."""
import numpy as np
import pytest

import sample_rows as S
from sample_ref import sample_row
from test_gpu_sample import EPS

N_HOT = 4096  # the grid of the GPU test at vocab <= 16411


def test_layouts_are_the_ones_the_rows_are_built_for():
    assert [S.layout(v) for v in S.VOCABS] == [(17, 2, 1), (1025, 65, 2), (2052, 129, 3), (32768, 2048, 32)]
    assert [v % 8 for v in S.VOCABS] == [3, 0, 3, 0]
    nvec, seg, _ = S.layout(131)
    assert [w for w in range(16) if w * seg >= nvec] == list(range(9, 16))  # waves 9 ... 15 own nothing
    # a launch holds 2^26 elements, give or take the 27 columns by which 16411 exceeds 2^14
    assert [S.grid_n(v) * (v & ~31) <= 2 ** 26 for v in S.VOCABS] == [True] * 4 and S.grid_n(16411) == N_HOT


def test_key_map():
    f = lambda *x: S.keys(np.array(x, np.float16)).tolist()  # noqa: E731
    assert f(0.0, -0.0, np.nan, -np.inf, np.inf) == [0x8000, 0x8000, 0, 0, 0xfc00]
    assert f(65504.0, -65504.0, 6e-8, -6e-8) == [0xfbff, 0x0400, 0x8001, 0x7ffe]
    every = np.arange(65536, dtype=np.uint16).view(np.float16)
    k, v = S.keys(every), every.astype(np.float64)
    fin = np.isfinite(v)
    order = np.argsort(v[fin], kind="stable")
    assert (np.diff(k[fin][order]) >= 0).all() and ((np.diff(k[fin][order]) == 0) == (np.diff(v[fin][order]) == 0)).all()
    assert k[fin].min() == 0x0400 and k[fin].max() == 0xfbff and (k[np.isnan(v)] == 0).all()


def test_hot_values():
    v, k = S.hot_values()
    x = v.astype(np.float64)
    assert v.size == 50 and x.min() == -1.5 and x.max() == 1.5 and (x * 4 == np.round(x * 4)).all()
    assert np.signbit(v[x == 0]).sum() == 1 and (x == 0).sum() >= 2  # -0 and +0: one tie group
    srt = np.sort(x)[::-1]
    assert srt[k - 1] == srt[k] and k == S.k_tie()
    key = S.keys(v)
    assert (key < 0x8000).any() and (key > 0x8000).any() and (key == 0x8000).sum() == (x == 0).sum()
    # multiples of 0.25: one value per key high byte (see the module's docstring)
    assert np.unique(key >> 8).size == np.unique(x).size


@pytest.mark.parametrize("vocab", S.VOCABS)
def test_hot_positions_and_filler(vocab):
    l, pos = S.sparse_row(vocab)
    nvec, seg, steps = S.layout(vocab)
    x = l.astype(np.float64)
    hot = np.zeros(vocab, bool)
    hot[pos] = True
    assert pos.size == 50 and np.unique(pos).size == 50
    assert sorted(x[pos].tolist()) == sorted(S.hot_values()[0].astype(np.float64).tolist())
    assert np.signbit(l[pos][x[pos] == 0]).sum() == 1
    must = [0, 7, 8, vocab - 1] + [8 * seg * w + d for w in range(1, 16) for d in (-1, 0) if 8 * seg * w + d < vocab]
    if seg > 64:
        must += [t for w in (0, 5, 15) for t in (8 * seg * w + 511, 8 * seg * w + 512) if t < vocab]
    if vocab > 8192:
        must += [8191, 8192]
    assert hot[must].all()
    # the filler: the four classes, all present, nothing else
    f = l[~hot]
    cls = [np.isneginf(f), np.isnan(f), f == np.float16(-30000), f == np.float16(-70)]
    assert all(c.sum() >= (vocab - 50) // 8 for c in cls) and np.logical_or.reduce(cls).all()
    # equal values lie in different waves, and past 8192 tokens in different histogram passes
    wave, hpass = pos // (8 * seg), pos // 8192
    for val in (-1.5, 0.0, 0.5):
        m = x[pos] == val
        assert np.unique(wave[m]).size >= 2, val
    if vocab > 8192:
        m = x[pos] == 0.5  # the tie at the k-th value
        assert np.unique(hpass[m]).size >= 2
    print(f"vocab {vocab}: nvec {nvec} seg {seg} steps {steps}, waves with a hot token {np.unique(wave).tolist()}, "
          f"passes {np.unique(hpass).tolist()}")


@pytest.mark.parametrize("vocab", S.VOCABS)
def test_cases_meet_what_the_gpu_tests_rely_on(vocab):
    """The branch of the kernel's top-p by the key high bytes of the two thresholds (every vocab alike, the hot values being the same):
    k+p at T = 0.5, 1, 2: 0xb8 (0.5, the k-th value) against 0xbc (1.0): DIFFERENT -- top-p walks level 2 once more for its own bin;
    k+plow at T = 0.5, 1, 2: 0xb8 against 0xb8: EQUAL -- top-p reuses top-k's level-2 histogram.  The cases p (no top-k threshold: always
    the extra walk), none, k and k60 (no top-p) have no such branch."""
    l, pos = S.sparse_row(vocab)
    key = S.keys(l)
    hot = np.zeros(vocab, bool)
    hot[pos] = True
    n = S.grid_n(vocab)
    u = S.u_grid(n)
    kt = S.k_tie()
    cases = S.cases(vocab)
    assert {(T, k, p == 1) for T, k, p, _ in cases} >= {(T, k, p1) for T in (0.5, 1.0, 2.0) for k, p1 in
                                                         ((0, True), (kt, True), (0, False), (kt, False), (60, True))}
    classes = set()
    for T, k, p, name in cases:
        r = S.sparse_ref(vocab, T, k, p)
        sh = r.survive & hot
        excluded = 1.0 - r.clear(u).mean()
        cls = "-"
        if k and p < 1:
            hk, hp = key[S.sparse_ref(vocab, T, k, np.float32(1)).survive].min() >> 8, key[r.survive].min() >> 8
            cls = "equal" if hk == hp else "different"
            classes.add(cls)
        print(f"vocab {vocab} {name:6s} T {T} k {k} p {float(p):.6f}: survivors {int(r.survive.sum())} ({int(sh.sum())} hot), excluded share "
              f"{excluded:.4f}, min hot prob * {N_HOT} = {r.prob[sh].min() * N_HOT:.2f} (* {n} = {r.prob[sh].min() * n:.2f}), "
              f"filler mass {r.prob[r.survive & ~hot].sum():.1e}, high bytes {cls}")
        assert r.prob[sh].min() > 2.0 / N_HOT
        assert r.prob[r.survive & ~hot].sum() <= 1e-8
        assert excluded <= 0.02
        assert not (r.survive & (key == 0)).any()
        if k == kt and p == 1:
            assert r.survive.sum() > k  # the tie at the k-th value is kept whole
        if name == "k+plow":
            assert (r.survive == S.sparse_ref(vocab, T, k, np.float32(1)).survive).all()
        if name in ("p", "k+p"):
            assert r.survive.sum() < S.sparse_ref(vocab, T, k, np.float32(1)).survive.sum()
        if k == 60:
            assert (r.survive & ~hot).any() and (r.prob[r.survive & ~hot] < 2.0 ** -44).all() and sh.sum() == 50
    assert classes == {"equal", "different"}


@pytest.mark.parametrize("vocab", S.VOCABS[:3])
def test_shared_reference_gives_sample_row_tokens(vocab):
    l, _ = S.sparse_row(vocab)
    u = S.u_grid(S.grid_n(vocab))[::97]
    for T, k, p, _ in S.cases(vocab)[:6]:
        r = S.sparse_ref(vocab, T, k, p)
        assert r.tokens(u).tolist() == [sample_row(l, T, k, p, x)["token"] for x in u]
        assert r.survive[r.tokens(u)].all()


def test_flat_and_two_level_rows():
    assert (S.flat_row(131, -3.5) == np.float16(-3.5)).all() and S.flat_row(131).shape == (131,)
    for abc, same_ab, same_bc in ((S.SAME_BYTE, True, False), (S.OTHER_BYTE, False, False), (S.ONE_BIN, True, True)):
        l = S.two_level_row(16411, abc)
        ka, kb, kc = S.keys(np.array(abc, np.float16)).tolist()
        assert ka > kb > kc and ((ka >> 8) == (kb >> 8)) == same_ab and ((kb >> 8) == (kc >> 8)) == same_bc
        x = l.astype(np.float64)
        assert (x[0::2] == abc[0]).all() and (x[15::16] == abc[2]).all() and (x == abc[1]).sum() == 16411 // 2 - 16411 // 16
        # log2 e / T_POW2 is a power of two exactly in f32, so the kernel's weights of these plateaus are exact powers of two
        s = S.POW2_SCALE[abc]
        assert S.LOG2E_F32 / np.float32(S.T_POW2[abc]) == np.float32(s)
        assert all(((v - abc[0]) * s) == round((v - abc[0]) * s) and (v - abc[0]) * s > -44 for v in abc)
    assert EPS == 1e-4
