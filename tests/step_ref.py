"""numpy restatement of one row of qqq_sample_advance's epilogue (include/qqq_amd_step.h): what the decode loop's state becomes once every
row's token of a step is known.  The tokens themselves are the sampler's (tests/sample_ref.py, ops.sample_tokens)."""
import numpy as np

FIELDS = ("tick", "ids", "pos", "slots", "remaining", "n_out", "out")


def new_state(rows, table_stride, out_stride, block_size):
    """An all-idle state: a dict of numpy arrays plus the scalar `block_size`."""
    return dict(tick=np.zeros(rows, np.int32), ids=np.zeros(rows, np.int64), pos=np.full(rows, -1, np.int64),
                slots=np.full(rows, -1, np.int64), block_table=np.zeros((rows, table_stride), np.int32),
                remaining=np.zeros(rows, np.int32), eos=np.full(rows, -1, np.int32), out=np.zeros((rows, out_stride), np.int64),
                n_out=np.zeros(rows, np.int32), block_size=int(block_size))


def copy_state(state):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}


def advance(state, tokens):
    """Apply one call to `state` in place, row by row, with `tokens[r]` the token row r drew.  Returns state."""
    bs = state["block_size"]
    table_stride, out_stride = state["block_table"].shape[1], state["out"].shape[1]
    for r, t in enumerate(tokens):
        t = int(t)
        state["tick"][r] += 1
        if state["remaining"][r] <= 0:
            continue
        n = int(state["n_out"][r])
        room = 0 <= n < out_stride
        if room:
            state["out"][r, n] = t
            state["n_out"][r] = n + 1
        rem = int(state["remaining"][r]) - 1
        if t == int(state["eos"][r]):
            rem = 0
        p = int(state["pos"][r]) + 1
        if not room or n + 1 >= out_stride or p < 0 or p // bs >= table_stride:
            rem = 0
        if rem > 0:
            state["ids"][r] = t
            state["pos"][r] = p
            state["slots"][r] = int(state["block_table"][r, p // bs]) * bs + p % bs
            state["remaining"][r] = rem
        else:
            state["ids"][r] = 0
            state["pos"][r] = -1
            state["slots"][r] = -1
            state["remaining"][r] = 0
    return state
