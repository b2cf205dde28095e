"""A deterministic corpus of drafter cases for qqq_spec_advance (include/qqq_amd_spec.h), numpy only.  A case is one row of a call: the
history before the call, the drafts the row was fed (ids[r, 1:]), the tokens of its G = K + 1 draws, and the PLAN: which match the
drafter must find in the history as it stands after the appends -- the depth n, the END position c = i + n - 1 of the earlier occurrence
and whether the draft copies its own output -- together with every other occurrence that was planted (`cands`), which a wrong scan would
pick instead.  tests/test_spec_corpus_cpu.py holds the corpus to its plans with spec_ref.advance and a search of its own;
tests/test_gpu_spec_scan.py runs the kernel on it.

The kernel's scan gives end position c to lane c % 256 (wave (c % 256) // 64) on pass c // 256, so the cases place matches by c: in
every wave, on the first pass, the second and a later one, alone and in competition.

How a history is planned.  Tokens 0 ... 15 are the alphabet of what is planted; filler is 16 + i % 985 at index i.  A history ends in the
gram 1 2 3 4 behind the separator 10.  An occurrence of depth d ending at c is the gram's last d tokens behind a filler token, followed
by a continuation token of its own: it matches the end of the history exactly d deep (min(d, ngram_max) under the cap), and since the
history's last token is of the alphabet and filler never is, filler matches nothing however often it repeats.  Runs (5 5 ... 5) give the
matches that end at c = L - 2, periods the overlapping copies.

The drafts a row was fed are an input of the call like any other (the rule compares the draws with ids[r, 1:], wherever they came from):
_emit() sets them so that exactly e draws are emitted -- the first e - 1 equal their draws, the next is WRONG, a token no draw has.  The
random sweep keeps the drafts of spec_ref.seat."""
import numpy as np

import spec_ref

HIST_STRIDE, BLOCK_SIZE, TABLE_STRIDE, VOCAB = 1100, 16, 72, 1003
GRAM, RUN, SEP, UNIQ, CONTS = [1, 2, 3, 4], 5, 10, 11, [6, 8, 9]
FILL0, FILL_N, WRONG, JUNK = 16, 985, 1001, 1002
IDLE = -7  # hist of the idle sentinel rows, and of every row behind its history
PAIRS = ((3, 4), (15, 4), (1, 1), (3, 2), (7, 3))  # the (draft_len, ngram_max) the corpus is laid out for
POSITIONS = (62, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 319, 320, 383, 384, 447, 448, 511, 512, 513, 575, 576, 639, 640, 703, 704, 767,
             1023)  # 383 ... 448 and 575 ... 704: waves 1 and 2 of the second and of a later pass
LENGTHS = (2, 3, 4, 5, 64, 65, 66, 256, 257, 258, 512, 513, 514, 1025, 1099)


def where(c):
    """(wave, pass class 0 / 1 / 2 for a later one) of the lane that scans end position c"""
    return (c % 256) // 64, min(c // 256, 2)


def _filler(n):
    return [FILL0 + i % FILL_N for i in range(n)]


def _plan(cands, length, k, nmax):
    """the winner among the planted occurrences (depth, c): the deepest under the cap, then the latest"""
    if not cands:
        return None
    n, c = max((min(d, nmax), c) for d, c in cands)
    return dict(n=n, c=c, overlap=c + k >= length)


def _emit(post, e, k):
    """-> (the history before the call, the drafts the row was fed, its draws) that append post[-e:] and nothing more"""
    n = len(post)
    assert 1 <= e <= k + 1 and n - e >= 1
    return post[:n - e], post[n - e + 1:] + [WRONG] * (k - e + 1), post[n - e:] + [JUNK] * (k + 1 - e)


def _case(name, group, post, cands, k, nmax, e=1, **kw):
    init, drafts, draws = _emit(post, e, k)
    plan = _plan(cands, len(post), k, nmax) if kw.get("goes_on", True) else None  # a row that retires drafts nothing
    return dict(dict(name=name, group=group, init=init, drafts=drafts, draws=draws, post=post, cands=list(cands), plan=plan, goes_on=True,
                     remaining=1000, pos=None, before=None, hist_len=None, pos0=None), **kw)


def _planted(length, plants):
    """filler, the occurrences (depth, c, continuation), the separator and the gram"""
    h = _filler(length)
    taken = set(range(length - 5, length))
    for d, c, cont in plants:
        cells = set(range(c - d, c + 2)) & set(range(length))  # the filler token in front, the occurrence, its continuation
        assert 1 <= d <= 4 and c - d + 1 >= 0 and not cells & taken, (length, plants)
        taken |= cells
        h[c - d + 1:c + 1] = GRAM[4 - d:]
        h[c + 1] = cont
    h[length - 5:] = [SEP] + GRAM
    return h


def _run(length, d):
    """a run of d + 1 tokens at the end: depth d at c = L - 2, whose draft is the run's token K times -- what no match at all gives too.
    So, where it fits, an earlier run of d tokens with another continuation: a scan that misses c = L - 2 drafts that one."""
    h = _filler(length)
    h[length - d - 1:] = [RUN] * (d + 1)
    cands = [(d, length - 2)]
    if length >= 2 * d + 2:
        h[:d + 1] = [RUN] * d + [CONTS[0]]
        cands.append((d, d - 1))
    return h, cands


def _positions(k, nmax):
    out = []
    for d in (1, 2, 3, 4):
        for c in (d - 1,) + POSITIONS:
            for length in (c + 7, 1090):  # just large enough, and long
                out.append(_case(f"pos-d{d}-c{c}-L{length}", "positions", _planted(length, [(d, c, CONTS[0])]), [(d, c)], k, nmax))
        for length in (2 * d + 2, 1090):
            h, cands = _run(length, d)
            out.append(_case(f"pos-d{d}-cL-2-L{length}", "positions", h, cands, k, nmax))
    return out


def _lengths(k, nmax):
    out = []
    for length in LENGTHS:
        h, cands = _run(length, 1)
        out.append(_case(f"len-{length}-match", "lengths", h, cands, k, nmax))
        out.append(_case(f"len-{length}-none", "lengths", _filler(length - 1) + [UNIQ], [], k, nmax))
    return out


def _largest_c(k, nmax, shift=0):
    """two occurrences of one depth: the later one wins.  Both orders of the continuations."""
    pairs = [("lane-pass0-pass1", 70, 326), ("lane-pass0-pass3", 70, 838), ("lane-pass1-pass2", 300, 556), ("waves-pass0", 10, 200),
             ("waves-pass1", 300, 500), ("wave1-lane63-pass0-wave2-lane0-pass1", 127, 384)]
    out = []
    for d in (1, 3):
        for tag, c0, c1 in pairs:
            for x, y in ((6, 8), (8, 6)):
                h = _planted(c1 + 7, [(d, c0, x), (d, c1, y)])
                out.append(_case(f"largest-d{d}-{tag}-{x}{y}", "largest_c", [t + shift for t in h], [(d, c0), (d, c1)], k, nmax))
    for c0 in (63, 127, 191, 255):  # neighbours: lane 63 of one wave and lane 0 of the next; depth 1 lets them touch
        for x in (6, 8):
            h = _planted(c0 + 8, [(1, c0 + 1, x)])
            h[c0] = GRAM[3]
            out.append(_case(f"largest-d1-neighbours-{c0}-{x}", "largest_c", [t + shift for t in h], [(1, c0), (1, c0 + 1)], k, nmax))
    return out


def _deepest(k, nmax):
    early, late = (20, 40, 60), (710, 730, 750)  # wave 0 of the first pass; wave 3 of the third
    out = []
    for tag, deep, shallow in (("deep-early", early[0], late[1:]), ("deep-late", late[2], early[:2])):
        plants = [(4, deep, 6), (1, shallow[0], 8), (2, shallow[1], 9)]
        out.append(_case(f"deepest-{tag}", "deepest", _planted(800, plants), [(d, c) for d, c, _ in plants], k, nmax))
    # ngram_max caps the depth: where the cap makes the two equal, the later one wins
    out.append(_case("cap-4-early-2-later", "cap", _planted(600, [(4, 30, 6), (2, 530, 8)]), [(4, 30), (2, 530)], k, nmax))
    return out


def _row_start(k, nmax):
    """hist[r, 0] is the history's last token, and the cells in front of it -- the end of the row above, an idle one -- go on like the
    history's end.  Inside the row, c = 0 matches one deep and loses to the later one-deep occurrence; a scan that stepped over the row's
    start would find it 2, 3, 4 deep (`false`), with another continuation."""
    out = []
    for length, c1 in ((40, 20), (300, 200)):
        for deep in (2, 3, 4):
            h = _planted(length, [(1, c1, 8)])
            h[0], h[1] = GRAM[3], 6
            out.append(_case(f"row-start-L{length}-false-{deep}-deep", "row_start", h, [(1, 0), (1, c1)], k, nmax,
                             before=[FILL0] + GRAM[4 - deep:3], false=[(min(deep, nmax), 0)]))
    return out


def _zeros(k, nmax):
    """histories shorter than ngram_max: the last tokens the kernel cannot read default to 0, and only c - t >= 0 keeps an all-zero
    history from matching them"""
    out = [_case(f"zeros-{n}", "zeros", [0] * n, [(n - 1, n - 2)], k, nmax) for n in (2, 3, 4, 5)]
    out.append(_case("zeros-7", "zeros", [0, 0, 7, 0, 0], [(2, 1), (1, 3)], k, nmax))
    return out


def _overlap(k, nmax):
    """a period of p ends the history: the match ends p before the end and the draft reads its own output (K = 15: 15, 7, 5, 3 times)"""
    out = []
    for p in (1, 2, 3, 5):
        for length in (255, 258, 511, 514):
            m = 2 * p + 4  # the periodic part: the match at distance p is four deep (so is the one at 2 p, which drafts the same)
            h = _filler(length - m) + [GRAM[i % p] if p < 5 else (GRAM + [RUN])[i % p] for i in range(m)]
            out.append(_case(f"overlap-p{p}-L{length}", "overlap", h, [(4, length - 1 - p)], k, nmax))
    return out


def _appends(k, nmax):
    """matches that exist only through what lane 0 appended in this call.  e = 1: the history's last token.  e = 2 and G, every draft
    accepted: a run of e tokens, so that the winning end position c = L - 2 is itself an appended cell, read by a lane of another wave."""
    out = []
    for length in (65, 66, 129, 130, 193, 194, 257, 258):
        out.append(_case(f"append-e1-L{length}", "appends", _planted(length, [(2, 12, 6)]), [(2, 12)], k, nmax))
        for e in sorted({2, k + 1}):
            h = [RUN, 6] + _filler(length - e)[2:] + [RUN] * e
            out.append(_case(f"append-e{e}-L{length}", "appends", h, [(e - 1, length - 2), (1, 0)], k, nmax, e=e))
    return out


def _unreachable(k, nmax):
    """remaining > 0 with a hist_len or a position no caller can leave behind: the row retires, nothing is appended or counted"""
    out = []
    for tag, kw in (("len0", dict(hist_len=0)), ("len-1", dict(hist_len=-1)), ("len-stride", dict(hist_len=HIST_STRIDE)),
                    ("len-stride+5", dict(hist_len=HIST_STRIDE + 5)), ("pos-1", dict(pos0=-1))):
        out.append(_case(f"unreachable-{tag}", "unreachable", _planted(40, [(2, 12, 6)]), [], k, nmax, goes_on=False, **kw))
    return out


def _sweep(k, nmax, rows=1500, seed=20):
    """random histories over 2, 3 and 8 symbols with the drafts spec_ref.seat gives them; the draws accept 0 ... K of those"""
    rng = np.random.default_rng(seed + 100 * k + nmax)
    out = []
    for i in range(rows):
        alphabet = (2, 3, 8)[i % 3]
        n = int(rng.integers(1, 1096))
        init = rng.integers(0, alphabet, n).tolist()
        drafts = spec_ref.draft(init, k, nmax)
        a = min(int(rng.integers(0, k + 1)), HIST_STRIDE - 2 - n)  # the history stays below hist_stride: the row goes on
        draws = drafts[:a] + rng.integers(0, alphabet, k + 1 - a).tolist()
        if a < k and draws[a] == drafts[a]:
            draws[a] = (drafts[a] + 1) % alphabet
        out.append(dict(name=f"sweep-{i}-a{alphabet}", group="sweep", init=init, drafts=None, draws=draws, post=init + draws[:a + 1], cands=None,
                        plan=None, goes_on=True, remaining=1000, pos=None, before=None, hist_len=None, pos0=None))
    return out


def _table_end(k, nmax, block_size, table_stride):
    """p' + K against the table's end, reached with 1 and with G tokens emitted; pos is independent of hist_len"""
    end = block_size * table_stride
    out = []
    for e in (1, k + 1):
        for tag, last in (("last-slot", end - 1), ("outside", end)):
            h = [RUN, 6] + _filler(60 - e)[2:] + [RUN] * e if e > 1 else _planted(60, [(2, 12, 6)])
            cands = [(e - 1, 58), (1, 0)] if e > 1 else [(2, 12)]
            out.append(_case(f"table-bs{block_size}-w{table_stride}-e{e}-{tag}", "table_end", h, cands, k, nmax, e=e, pos=last - k - e,
                             goes_on=last < end))
    return out


def layout(groups, k, nmax, block_size=BLOCK_SIZE, table_stride=TABLE_STRIDE, seed=1):
    """One state of R rows for the cases of `groups` (lists of cases): an idle sentinel row first, last and between the groups, and one in
    front of every case that wants the cells above it set (`before`).  -> dict(state, draws [R][G], cases {row: case}, idle [rows],
    block_size, ngram_max)"""
    order = [None]
    for g in groups:
        for case in g:
            if case["before"] is not None:
                order.append(case["before"])
            order.append(case)
        order.append(None)
    rows = len(order)
    assert rows * (k + 1) <= 65535
    rng = np.random.default_rng(seed)
    st = spec_ref.new_state(rows, k, table_stride, HIST_STRIDE, block_size)
    st["block_table"][:] = rng.integers(0, 4096, (rows, table_stride))
    st["tick"][:] = np.arange(rows) % 3
    st["hist"][:] = IDLE
    draws = np.full((rows, k + 1), JUNK, np.int64)
    cases, idle = {}, []
    for r, item in enumerate(order):
        if not isinstance(item, dict):
            idle.append(r)
            if item is not None:
                st["hist"][r, HIST_STRIDE - len(item):] = item
            continue
        cases[r] = item
        spec_ref.seat(st, r, item["init"], st["block_table"][r].copy(), item["remaining"], nmax, pos=item["pos"])
        if item["drafts"] is not None:
            st["ids"][r, 1:] = item["drafts"]
        if item["hist_len"] is not None:
            st["hist_len"][r] = item["hist_len"]
        if item["pos0"] is not None:
            st["pos"][r, 0] = item["pos0"]
        draws[r] = item["draws"]
    return dict(state=st, draws=draws, cases=cases, idle=idle, block_size=block_size, ngram_max=nmax)


def planned(k, nmax):
    """the planned groups of the main geometry"""
    return [f(k, nmax) for f in (_positions, _lengths, _largest_c, _deepest, _row_start, _zeros, _overlap, _appends, _unreachable)]


def batches(k, nmax, sweep_rows=1500):
    """the whole corpus for (draft_len, ngram_max) as calls: the main geometry with the planned groups and the random sweep, then one
    small call per (block_size, table_stride) of the table-end cases"""
    out = [layout(planned(k, nmax) + [_sweep(k, nmax, sweep_rows)], k, nmax)]
    for bs in (16, 256):
        for width in (2, 5):
            out.append(layout([_table_end(k, nmax, bs, width)], k, nmax, bs, width))
    return out


def top_of_vocab(k, nmax, vocab=262144):
    """a few rows whose token ids sit just below `vocab`: the largest-c cases moved up"""
    return layout([[c for c in _largest_c(k, nmax, vocab - VOCAB) if "-d3-" in c["name"]][:8]], k, nmax)
