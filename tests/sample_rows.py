"""Rows of logits that put ops.sample_tokens (include/qqq_amd_sample.h) past one wave, one histogram pass and one bin, numpy only; the
kernel's key map restated; and the reference of a (row, T, k, p) case computed once and shared.  tests/test_sample_rows_cpu.py holds the
rows to their conditions with tests/sample_ref.py alone; tests/test_gpu_sample_rows.py runs the kernel on them.

How the kernel lays a row out (qqq_amd/csrc/qqq_sample.hip.h): nvec = ceil(vocab / 8) vectors of 8 tokens.  The histogram walks give vector
v to thread v % 1024 on pass v // 1024, so tokens from 8192 on are a second pass.  The draw gives wave w of 16 the vectors
[w seg, (w + 1) seg), seg = ceil(nvec / 16), and walks them 64 vectors (512 tokens) per step.

sparse_row: the 50 values of test_gpu_sample._grid_row() shifted by -1.5 -- multiples of 0.25 in [-1.5, 1.5], keys on both sides of 0x8000,
one of the zeros as -0 -- at the first and last token of waves, draw steps and histogram passes; every other token is filler without
weight.  In fp16 a multiple of 0.25 of this range has a zero low byte, so each hot value has a key high byte of its own and a top-p cut in
the top-k threshold's level-1 bin is a cut in that threshold's own tie group (p "low" of cases()); two_level_row holds the plateaus that
share a high byte and differ in the low one.
"""
import functools

import numpy as np

from sample_ref import sample_row
from test_gpu_sample import EPS, _grid_row, _top_p_in_the_widest_gap

VOCABS = (131, 8200, 16411, 262144)
TS = (0.5, 1.0, 2.0)
FILLER = (-np.inf, np.nan, -30000.0, -70.0)  # no weight; no weight; weight exactly 0; weight below 2^-44 in the kernel, ~0 in float64
MIN_GAP = 4e-3
LOG2E_F32 = np.float32(1.4426950408889634)


def grid_n(vocab):
    """rows of a u grid: about 2^26 elements per launch at the most"""
    return 4096 if vocab <= 16411 else 256


def layout(vocab):
    nvec = (vocab + 7) // 8
    seg = (nvec + 15) // 16
    return nvec, seg, (seg + 63) // 64


def keys(l):
    """the unsigned key of every fp16 logit, as the header comment of qqq_sample.hip.h states it: it orders like the value, -0 joins +0,
    NaN and -inf are key 0, finite values 0x0400 ... 0xfbff, +inf 0xfc00"""
    b = np.asarray(l, np.float16).view(np.uint16).astype(np.int64)
    key = np.where(b & 0x8000, ~b & 0xffff, b | 0x8000)
    key = np.where(b == 0x8000, 0x8000, key)
    return np.where(((b & 0x7fff) > 0x7c00) | (b == 0xfc00), 0, key)


def hot_values():
    """-> (the 50 hot values fp16, k with a tie at the k-th largest)"""
    l, k = _grid_row()
    v = (l.astype(np.float64) - 1.5).astype(np.float16)
    zeros = np.nonzero(v == 0)[0]
    assert zeros.size >= 2
    v[zeros[0]] = np.float16(-0.0)
    return v, k


def hot_positions(vocab, rng):
    nvec, seg, _ = layout(vocab)
    want = [0, 7, 8, vocab - 1]
    for w in range(1, 16):
        want += [8 * seg * w - 1, 8 * seg * w]
    if seg > 64:
        for w in (0, 5, 15):
            want += [8 * seg * w + 511, 8 * seg * w + 512]
    if vocab > 8192:
        want += [8191, 8192]
    pos = sorted({t for t in want if 0 <= t < vocab})
    assert len(pos) <= 50 <= vocab
    rest = np.setdiff1d(np.arange(vocab), pos)
    return np.sort(np.concatenate([pos, rng.choice(rest, 50 - len(pos), replace=False)]).astype(np.int64))


@functools.lru_cache(maxsize=None)
def _sparse(vocab, seed):
    rng = np.random.default_rng([vocab, seed])
    vals, k = hot_values()
    pos = hot_positions(vocab, rng)
    l = np.array(FILLER, np.float16)[rng.integers(0, 4, vocab)]
    vals = vals[rng.permutation(50)]
    if vocab > 8192:  # one of the ties at the k-th value starts the second histogram pass, whatever the permutation
        kth = np.sort(vals.astype(np.float64))[50 - k]
        i, j = int(np.nonzero(pos == 8192)[0][0]), int(np.nonzero(vals == kth)[0][0])
        vals[[i, j]] = vals[[j, i]]
    l[pos] = vals
    l.setflags(write=False)
    pos.setflags(write=False)
    return l, pos, k


def sparse_row(vocab, seed=0):
    """-> (logits fp16 [vocab], the 50 hot positions ascending); read-only, shared"""
    return _sparse(vocab, seed)[:2]


def k_tie():
    return hot_values()[1]


def flat_row(vocab, value=0.0):
    return np.full(vocab, value, np.float16)


# plateaus (a, b, c): keys 0xc080 0xc000 0xbc00; 0xc000 0xbe00 0xbc00; 0xc0c0 0xc080 0xc000 (all three in one level-1 bin)
SAME_BYTE, OTHER_BYTE, ONE_BIN = (2.25, 2.0, 1.0), (2.0, 1.5, 1.0), (2.375, 2.25, 2.0)
# the scale log2 e / T at which the kernel's weights of these plateaus are exact powers of two, and that T (the f32 quotient is exact)
POW2_SCALE = {SAME_BYTE: 4, OTHER_BYTE: 4, ONE_BIN: 8}
T_POW2 = {abc: float(np.float32(LOG2E_F32 / np.float32(s))) for abc, s in POW2_SCALE.items()}


def two_level_row(vocab, abc=SAME_BYTE):
    """even tokens a, odd tokens b < a, and the lower plateau c on every 16th token (15, 31, ...)"""
    a, b, c = abc
    l = np.where(np.arange(vocab) % 2 == 0, a, b).astype(np.float16)
    l[15::16] = c
    return l


# ---- the cases of a sparse row and their reference, computed once

def tie_group_edges(l, T, k):
    """the cumulative masses of the tie groups of the top-k set, from the least probable up, as fractions of W: 0, ..., 1.  Group g
    survives a top-p with 1 - p below edge g + 1."""
    base = sample_row(l, T, k, 1.0, 0.0)
    w = np.diff(np.concatenate([[0.0], base["c"]]))
    s = base["survive"]
    vals, inv = np.unique(l[s].astype(np.float64), return_inverse=True)
    return np.concatenate([[0.0], np.cumsum(np.bincount(inv, weights=w[s], minlength=vals.size)) / w.sum()])


def _tie_group_gaps(l, T, k):
    """(p at the middle of the gap, the gap) for every tie group of the top-k set, from the least probable up"""
    cum = tie_group_edges(l, T, k)
    return [(np.float32(1.0 - 0.5 * (lo + hi)), float(hi - lo)) for lo, hi in zip(cum[:-1], cum[1:])]


@functools.lru_cache(maxsize=None)
def cases(vocab, seed=0):
    """-> tuple of (T, k, p, name): T x {none, k, p, k + p, k = 60}, and k with p "low": a cut in the middle of the k-th value's own tie
    group, which keeps the whole top-k set through the kernel's reuse of top-k's level-2 histogram"""
    l, _, kt = _sparse(vocab, seed)
    out = []
    for T in TS:
        out.append((T, 0, np.float32(1), "none"))
        out.append((T, kt, np.float32(1), "k"))
        for k, name in ((0, "p"), (kt, "k+p")):
            p, gap = _top_p_in_the_widest_gap(l, T, k)
            assert gap >= MIN_GAP, (vocab, T, k, gap)
            out.append((T, k, p, name))
        out.append((T, 60, np.float32(1), "k60"))
        # _top_p_in_the_widest_gap never cuts the lowest kept group (it wants a lower edge above 0.05), and every other group has another
        # key high byte than the top-k threshold: the one gap in that threshold's bin is its own group's
        p, gap = _tie_group_gaps(l, T, kt)[0]
        assert gap >= MIN_GAP, (vocab, T, gap)
        out.append((T, kt, p, "k+plow"))
    return tuple(out)


class Ref:
    """the reference of one (row, T, k, p): the surviving set, the probabilities, the edges c_j / W2 and the token of any u"""

    def __init__(self, l, T, k, p):
        r = sample_row(l, T, k, p, 0.0)
        self.survive, self.c, self.W2 = r["survive"], r["c"], r["W2"]
        self.prob = np.diff(np.concatenate([[0.0], self.c])) / self.W2
        self.edges = np.unique(self.c[self.survive]) / self.W2

    def tokens(self, u):
        """sample_row(...)["token"] for every u of an f32 array in [0, 1): the lowest j with c_j > u W2, which is a survivor"""
        x = np.asarray(u, np.float32).astype(np.float64) * self.W2
        return np.searchsorted(self.c, x, side="right")

    def clear(self, u):
        """whether each u lies farther than EPS from every edge (and from 0)"""
        e = np.concatenate([[0.0], self.edges])
        u = np.asarray(u, np.float64)
        i = np.clip(np.searchsorted(e, u), 1, e.size - 1)
        return np.minimum(np.abs(u - e[i - 1]), np.abs(u - e[i])) > EPS


@functools.lru_cache(maxsize=None)
def sparse_ref(vocab, T, k, p, seed=0):
    return Ref(_sparse(vocab, seed)[0], T, k, p)


def u_grid(n):
    return ((np.arange(n) + 0.5) / n).astype(np.float32)
