"""ops.ban_tokens and ops.stop_check on the GPU against tests/stop_ref.py, on hand-made states: every array the ops write is compared
whole, so a row that must stay untouched is held to that too.  Integer work: every comparison is exact."""
import numpy as np
import pytest
import torch

import stop_ref

pytestmark = pytest.mark.gpu

VOCAB, LD = 1003, 1008


# ---- ban_tokens

def _ban_case(rows, g, base, seed):
    """rows whose first logits row sits 0 ... g + 1 indices below the row's minimum: offset k bans the logits rows j < k, so row k - 1 is at
    index exactly min_new - 1 and row k at exactly min_new"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(-32768, 32768, size=(rows * g, LD), dtype=np.int64).astype(np.int16)  # any bit pattern, NaNs included
    n_out = rng.integers(0, 10, size=rows).astype(np.int32)
    min_new = (n_out + base + np.arange(rows) % (g + 2)).astype(np.int32)
    eos = rng.integers(0, VOCAB, size=rows).astype(np.int32)
    eos[::3] = -1
    eos[1] = VOCAB  # out of range: ignored
    ban = np.array([5, VOCAB - 1, 5, -5, VOCAB, 2_000_000, 0, 17, 17, VOCAB + 4], np.int32)  # duplicates, ids out of range, the padding columns
    return bits, n_out, min_new, eos, ban


@pytest.mark.parametrize("rows", [3, 70])
@pytest.mark.parametrize("g", [1, 5])
@pytest.mark.parametrize("base", [0, 1])
def test_ban_tokens_equals_the_reference_bit_for_bit(dev, rows, g, base):
    from qqq_amd import ops

    bits, n_out, min_new, eos, ban = _ban_case(rows, g, base, rows * 10 + g)
    want = bits.copy()
    stop_ref.ban_tokens(want.view(np.float16), n_out, min_new, eos, ban, base, vocab=VOCAB)
    assert (want != bits).any() and (want[:, VOCAB:] == bits[:, VOCAB:]).all()
    banned = (want != bits).any(axis=1).reshape(rows, g)
    assert not banned[0].any() and banned[1, 0] and (g == 1 or (banned[2, :2].all() and not banned[2, 2]))
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    full = t(bits).view(torch.float16)
    logits = full[:, :VOCAB]  # a view of the wider matrix: rewritten in place
    assert ops.ban_tokens(logits, t(n_out), t(min_new), t(eos), t(ban), base=base) is logits
    assert np.array_equal(full.view(torch.int16).cpu().numpy(), want)
    # no ban ids: the eos alone
    want = bits.copy()
    stop_ref.ban_tokens(want.view(np.float16), n_out, min_new, eos, [], base, vocab=VOCAB)
    full = t(bits).view(torch.float16)
    ops.ban_tokens(full[:, :VOCAB], t(n_out), t(min_new), t(eos), None, base=base)
    assert np.array_equal(full.view(torch.int16).cpu().numpy(), want)


# ---- stop_check

SEQ32 = [(7 * i + 3) % 11 + 20 for i in range(32)]
# the table of the hand-made rows: a length-1, two length-2 (the second also matches where the first does not), the same length-2 again
# at a higher index, a length-32, and an unused entry in between
TABLE = [[9], [4, 5], [6, 5], [], [4, 5], SEQ32, [15, 4, 5], [6, 31], [31]]
END_IDS = [-1, 13, 9_999]

EOS = 31  # the eos of every hand-made row; the random rows behind them have none

# (completion, n_seen, min_new, remaining before) -> what must come out (n_trim, stop_hit) or None for no match
HAND = [
    (([1, 2, 4, 5, 3], 2, 0, 4), (1 + 2, 1)),            # three new ends, the second matches
    (([1, 15, 4, 5], 3, 0, 4), (0 + 2, 1)),              # two sequences (and a third at a higher index) match at one end: the lowest wins
    ((SEQ32, 31, 0, 4), (32, 5)),                        # length 32 spanning the whole completion, its first token included
    (([4, 5], 1, 0, 4), (2, 1)),                         # a match that spans the first token
    (([1, 4, 5], 3, 0, 4), None),                        # nothing new (n_seen == m): untouched although it ends in a stop
    (([9], 1, 0, 0), None),                              # idle
    (([5], 0, 0, 4), None),                              # L > e: [4, 5] and [6, 5] end in the token, the completion is too short
    (([4, 5, 1], 1, 3, 4), None),                        # the match ends at 2, below the minimum of 3
    (([4, 5, 9], 1, 3, 4), (1, 0)),                      # ... and the end at the minimum is tested
    (([1, 2, 6, 5], 3, 0, 0), (2, 2)),                   # a row that eos or the budget retired in this step is still checked
    (([1, 13, 2], 1, 0, 4), (1, 32 + 1)),                # an end id: the token stays
    (([1, 9, 13], 2, 0, 4), (0, 32 + 1)),                # at the end checked
    (([2, 3, 9, 4, 5], 0, 0, 4), (2 + 1, 0)),            # the earliest end wins over a later, longer match
    (([1, 6, 31], 1, 0, 0), (0, 32 + 3)),                # the row's eos goes before a sequence that ends in it ([6, 31], [31]): the token stays
    (([31], 0, 0, 0), (0, 32 + 3)),                      # ... as the first token
    (([1, 31, 2], 1, 5, 0), (1, 32 + 3)),                # ... and below the minimum, where no sequence is tested
    (([1, 13], 1, 5, 4), (0, 32 + 1)),                   # an end id below the minimum
]


def _layout(rows_spec, dtype, g, n_stop, table, rows=None, stride=40, seed=0):
    """the hand-made completions in one of the two addressings: int64 = DecodeLoop's (`first`, then out), int32 = SpecDecodeLoop's (behind
    a prompt in hist) -> the numpy state stop_ref.stop_check takes"""
    rng = np.random.default_rng(seed)
    rows = len(rows_spec) if rows is None else rows
    spec = list(rows_spec) + [([int(x) for x in rng.integers(0, 3, size=int(rng.integers(1, 13)))], None, int(rng.integers(0, 4)), 3)
                              for _ in range(rows - len(rows_spec))]
    tokens = rng.integers(0, 3, size=(rows, stride)).astype(dtype)
    base, first = np.zeros(rows, np.int32), np.zeros(rows, np.int32)
    n_out, n_seen, min_new, remaining = (np.zeros(rows, np.int32) for _ in range(4))
    for r, (c, seen, least, rem) in enumerate(spec):
        m = len(c)
        if dtype == np.int64:
            base[r], first[r] = -1, c[0]
            tokens[r, :m - 1] = c[1:]
        else:
            base[r] = 3 + r % 4
            tokens[r, base[r]:base[r] + m] = c
        n_out[r], min_new[r], remaining[r] = m - 1, least, rem
        n_seen[r] = int(rng.integers(0, m + 1)) if seen is None else seen
    stop_ids = rng.integers(0, 3, size=(n_stop, 32)).astype(np.int32)
    stop_len = np.zeros(n_stop, np.int32)
    for s, seq in enumerate(table[:n_stop]):
        stop_ids[s, :len(seq)], stop_len[s] = seq, len(seq)
    live = remaining > 0
    eos = np.full(rows, -1, np.int32)
    eos[:len(rows_spec)] = EOS
    per = lambda v: (v if g == 0 else np.repeat(v[:, None], g, axis=1)).astype(np.int64)  # noqa: E731
    return dict(tokens=tokens, base=base, first=first if dtype == np.int64 else None, n_out=n_out, stop_ids=stop_ids, stop_len=stop_len,
                min_new=min_new, n_seen=n_seen, n_trim=np.full(rows, -7, np.int32), stop_hit=np.full(rows, -7, np.int32),
                ids=per(np.where(live, 5, 0)), pos=per(np.where(live, 11, -1)), slots=per(np.where(live, 27, -1)), remaining=remaining,
                start=None if dtype == np.int64 else np.where(live, 11, -1).astype(np.int64), eos=eos)


WRITTEN = ("n_seen", "n_trim", "stop_hit", "ids", "pos", "slots", "remaining", "start")


def _run(dev, st, end_ids):
    from qqq_amd import ops

    gpu = {k: None if v is None else torch.from_numpy(v.copy()).to(dev) for k, v in st.items()}
    ops.stop_check(**gpu, end_ids=None if end_ids is None else torch.tensor(end_ids, dtype=torch.int32, device=dev))
    want = {k: None if v is None else v.copy() for k, v in st.items()}
    stop_ref.stop_check(**want, end_ids=end_ids or [])
    for k in st:
        if st[k] is not None:
            assert np.array_equal(gpu[k].cpu().numpy(), want[k]), k
            assert k in WRITTEN or np.array_equal(want[k], st[k]), k  # the inputs are only read
    return want


@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["out64", "hist32"])
def test_stop_check_on_hand_made_rows(dev, dtype):
    g = 0 if dtype == np.int64 else 4
    st = _layout([h[0] for h in HAND], dtype, g, 32, TABLE)
    want = _run(dev, st, END_IDS)
    for r, ((c, seen, least, rem), out) in enumerate(HAND):
        m = len(c)
        if out is None:
            assert (want["n_trim"][r], want["stop_hit"][r], want["remaining"][r]) == (-7, -7, rem), r
            assert want["n_seen"][r] == (seen if seen >= m else m), r
        else:
            assert (want["n_trim"][r], want["stop_hit"][r], want["remaining"][r], want["n_seen"][r]) == (*out, 0, m), r
            assert (want["pos"][r] == -1).all() and (want["slots"][r] == -1).all() and (want["ids"][r] == 0).all(), r
            assert dtype == np.int64 or want["start"][r] == -1
    # without the eos array the sequences that end in that token cut the same rows: the argument is what decides
    bare = _run(dev, dict(st, eos=None), END_IDS)
    at = [r for r, (h, _) in enumerate(HAND) if h[0] in ([1, 6, 31], [31])]
    assert bare["n_trim"][at].tolist() == [2, 1] and bare["stop_hit"][at].tolist() == [7, 8]
    # five rows, two of them idle, one sequence: n_stop = 1
    st = _layout([HAND[0][0], HAND[4][0], HAND[3][0], HAND[5][0], HAND[6][0]], dtype, g, 1, [[4, 5]])
    want = _run(dev, st, None)
    assert want["n_trim"].tolist() == [3, -7, 2, -7, -7] and want["stop_hit"].tolist() == [0, -7, 0, -7, -7]
    assert want["n_seen"].tolist() == [5, 3, 2, 1, 1]


@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["out64", "hist32"])
@pytest.mark.parametrize("n_stop,g", [(1, 0), (32, 1), (32, 16)])
def test_stop_check_on_70_rows_equals_the_reference(dev, dtype, n_stop, g):
    """random completions over three tokens behind the hand-made rows, random n_seen and minimums: sequences of lengths 1 ... 5 and 32
    match in some rows and not in others"""
    rng = np.random.default_rng(n_stop + g)
    table = TABLE + [[int(x) for x in rng.integers(0, 3, size=int(rng.integers(3, 6)))] for _ in range(32 - len(TABLE))]
    st = _layout([h[0] for h in HAND], dtype, g, n_stop, table if n_stop == 32 else [[1, 2]], rows=70, seed=n_stop * 100 + g)
    want = _run(dev, st, END_IDS if n_stop == 32 else [2])
    hit = want["stop_hit"] != -7
    checked = st["n_seen"] < st["n_out"] + 1
    assert 5 <= hit.sum() <= checked.sum() - 5 and (want["n_seen"][checked] == st["n_out"][checked] + 1).all()
    assert (want["n_seen"][~checked] == st["n_seen"][~checked]).all() and not hit[~checked].any()


def test_both_ops_replay_from_a_graph_with_changed_contents(dev):
    from qqq_amd import ops

    t = lambda a: None if a is None else torch.from_numpy(a.copy()).to(dev)  # noqa: E731
    st = _layout([h[0] for h in HAND], np.int32, 4, 32, TABLE, rows=20, seed=1)
    end = torch.tensor(END_IDS, dtype=torch.int32, device=dev)
    bits, n_out, min_new, eos, ban = _ban_case(20, 4, 1, 3)
    held = {k: t(v) for k, v in st.items()}
    ban_held = dict(full=t(bits).view(torch.float16), n_out=t(n_out), min_new=t(min_new), eos=t(eos), ban=t(ban))

    def step():
        ops.ban_tokens(ban_held["full"][:, :VOCAB], ban_held["n_out"], ban_held["min_new"], ban_held["eos"], ban_held["ban"], base=1)
        ops.stop_check(**held, end_ids=end)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    # other contents in the same arrays: the rows in another order, another table, other logits and counts
    order = np.random.default_rng(5).permutation(len(HAND))
    st2 = _layout([HAND[i][0] for i in order], np.int32, 4, 32, TABLE[::-1], rows=20, seed=2)
    bits2, n_out2, min_new2, eos2, ban2 = _ban_case(20, 4, 1, 4)
    for k, v in st2.items():
        if v is not None:
            held[k].copy_(t(v))
    for k, v in (("full", bits2.view(np.float16)), ("n_out", n_out2), ("min_new", min_new2), ("eos", eos2), ("ban", ban2[::-1].copy())):
        ban_held[k].copy_(t(v))
    graph.replay()
    torch.cuda.synchronize(dev)
    want = {k: None if v is None else v.copy() for k, v in st2.items()}
    stop_ref.stop_check(**want, end_ids=END_IDS)
    for k in WRITTEN:
        assert np.array_equal(held[k].cpu().numpy(), want[k]), k
    assert (want["stop_hit"] != -7).sum() >= 5
    want_bits = bits2.copy()
    stop_ref.ban_tokens(want_bits.view(np.float16), n_out2, min_new2, eos2, ban2, 1, vocab=VOCAB)
    assert np.array_equal(ban_held["full"].view(torch.int16).cpu().numpy(), want_bits) and (want_bits != bits2).any()
