"""numpy / Python restatement of one call of qqq_spec_advance (include/qqq_amd_spec.h): the n-gram draft rule and what the speculative decode
loop's state becomes once every draw of a step is known.  The draws themselves are the sampler's (tests/sample_ref.py, ops.sample_tokens).
Written from the header's statement, independently of qqq_amd.serve.ngram_draft."""
import numpy as np

FIELDS = ("tick", "ids", "pos", "slots", "start", "remaining", "hist", "hist_len", "n_out", "n_acc")


def draft(history, draft_len, ngram_max):
    """d_0 ... d_{K-1}: for n = ngram_max ... 1 (only n < L) the largest i < L - n whose n-gram equals the last n tokens; the first n with a
    match wins; the draft continues the sequence from i + n, reading its own output once it passes the end (the overlapping copy).  No
    match: the last token, K times."""
    h = [int(t) for t in history]
    L = len(h)
    assert L >= 1
    for n in range(ngram_max, 0, -1):
        if not n < L:
            continue
        where = [i for i in range(L - n) if h[i:i + n] == h[L - n:]]
        if where:
            grown = list(h)
            for j in range(draft_len):
                grown.append(grown[max(where) + n + j])
            return grown[L:]
    return [h[L - 1]] * draft_len


def new_state(rows, draft_len, table_stride, hist_stride, block_size):
    """An all-idle state: a dict of numpy arrays plus the scalars `block_size` and `draft_len`."""
    g = draft_len + 1
    return dict(tick=np.zeros(rows, np.int32), ids=np.zeros((rows, g), np.int64), pos=np.full((rows, g), -1, np.int64),
                slots=np.full((rows, g), -1, np.int64), start=np.full(rows, -1, np.int64),
                block_table=np.zeros((rows, table_stride), np.int32), remaining=np.zeros(rows, np.int32), eos=np.full(rows, -1, np.int32),
                hist=np.zeros((rows, hist_stride), np.int32), hist_len=np.zeros(rows, np.int32), n_out=np.zeros(rows, np.int32),
                n_acc=np.zeros(rows, np.int32), block_size=int(block_size), draft_len=int(draft_len))


def copy_state(state):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}


def seat(state, r, history, blocks, remaining, ngram_max, eos=-1, pos=None):
    """Make row r active with `history` (its last token is the row's next input) over the cache blocks `blocks`: what a host does at
    admission.  `pos`: the position of the last token, len(history) - 1 unless given."""
    bs, k = state["block_size"], state["draft_len"]
    n = len(history)
    first = n - 1 if pos is None else int(pos)
    state["hist"][r, :n] = history
    state["hist_len"][r] = n
    state["block_table"][r, :len(blocks)] = blocks
    state["ids"][r] = [history[-1]] + draft(history, k, ngram_max)
    for j in range(k + 1):
        q = first + j
        state["pos"][r, j] = q
        state["slots"][r, j] = int(state["block_table"][r, q // bs]) * bs + q % bs
    state["start"][r] = first
    state["remaining"][r] = remaining
    state["eos"][r] = eos
    state["n_out"][r] = state["n_acc"][r] = 0


def advance(state, tokens, ngram_max):
    """Apply one call to `state` in place, row by row, with tokens[r][j] the token of draw j of row r.  Returns state."""
    bs, k = state["block_size"], state["draft_len"]
    table_stride, hist_stride = state["block_table"].shape[1], state["hist"].shape[1]
    for r in range(state["tick"].shape[0]):
        state["tick"][r] += 1
        if state["remaining"][r] <= 0:
            continue
        rem, p, n = int(state["remaining"][r]), int(state["pos"][r, 0]), int(state["hist_len"][r])
        alive = p >= 0 and 1 <= n < hist_stride  # anything else is state no caller can reach: retire, append nothing
        if alive:
            emitted = 0
            for j in range(k + 1):
                if n >= hist_stride:  # no room: not appended, and the row retires
                    alive = False
                    break
                s = int(tokens[r][j])
                state["hist"][r, n] = s
                n += 1
                emitted += 1
                state["n_out"][r] += 1
                rem -= 1
                if s == int(state["eos"][r]) or rem <= 0:
                    alive = False
                    break
                if j == k or s != int(state["ids"][r, j + 1]):
                    break
                state["n_acc"][r] += 1
            state["hist_len"][r] = n
            p += emitted  # the position of the last emitted token
            if n >= hist_stride or (p + k) // bs >= table_stride:
                alive = False
        if alive:
            state["ids"][r] = [int(state["hist"][r, n - 1])] + draft(state["hist"][r, :n], k, ngram_max)
            for j in range(k + 1):
                state["pos"][r, j] = p + j
                state["slots"][r, j] = int(state["block_table"][r, (p + j) // bs]) * bs + (p + j) % bs
            state["start"][r] = p
            state["remaining"][r] = rem
        else:
            state["ids"][r] = 0
            state["pos"][r] = -1
            state["slots"][r] = -1
            state["start"][r] = -1
            state["remaining"][r] = 0
    return state
