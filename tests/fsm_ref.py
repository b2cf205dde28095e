"""numpy reference of the two guided-decoding ops, written from the rules in include/qqq_amd_guided.h: integer and bit work, so a
test compares with equality.  Logits are uint16 bit patterns of fp16 values; every array is updated in place."""
import numpy as np

NEG_INF = 0xFC00


def _bounds(offsets, s, n_edges):
    """lo(s), hi(s): both offsets clamped into [0, n_edges], an end below its begin is an empty list"""
    lo = min(max(int(offsets[s]), 0), n_edges)
    hi = min(max(int(offsets[s + 1]), 0), n_edges)
    return lo, max(lo, hi)


def mask(logits, state, offsets, tokens, accept, eos=None, remaining=None, vocab=None):
    """logits uint16 [rows, ld] (ld >= vocab; vocab None: every column)"""
    assert logits.dtype == np.uint16 and logits.ndim == 2
    vocab = logits.shape[1] if vocab is None else vocab
    n_states, n_edges = len(accept), len(tokens)
    for r in range(logits.shape[0]):
        s = int(state[r])
        if not 0 <= s < n_states or (remaining is not None and remaining[r] == 0):
            continue
        lo, hi = _bounds(offsets, s, n_edges)
        keep = np.zeros(vocab, dtype=bool)
        allowed = np.asarray(tokens[lo:hi], dtype=np.int64)
        keep[allowed[(allowed >= 0) & (allowed < vocab)]] = True
        if eos is not None and accept[s] != 0 and 0 <= int(eos[r]) < vocab:
            keep[int(eos[r])] = True
        logits[r, :vocab][~keep] = NEG_INF
    return logits


def advance(out, n_out, n_fsm, state, offsets, tokens, next, accept, ids, pos, slots, remaining, eos=None):  # noqa: A002
    n_states, n_edges = len(accept), len(tokens)
    for r in range(out.shape[0]):
        m = int(n_out[r])
        if int(n_fsm[r]) >= m:
            continue
        retire = False
        for i in range(max(int(n_fsm[r]), 0), m):
            if i >= out.shape[1]:
                break
            s, t = int(state[r]), int(out[r, i])
            if not 0 <= s < n_states:  # rule 1
                continue
            lo, hi = _bounds(offsets, s, n_edges)
            edge = lo + np.nonzero(np.asarray(tokens[lo:hi], dtype=np.int64) == t)[0]
            if edge.size:  # rule 2
                to = int(next[edge[0]])
                if not 0 <= to < n_states:
                    state[r], retire = -2, True
                else:
                    state[r] = to
                    lo2, hi2 = _bounds(offsets, to, n_edges)
                    retire = retire or lo2 == hi2
            elif accept[s] != 0 and eos is not None and t == int(eos[r]) >= 0:  # rule 3
                pass
            else:  # rule 4
                state[r], retire = -2, True
        n_fsm[r] = m
        if retire:
            ids[r], pos[r], slots[r], remaining[r] = 0, -1, -1, 0
