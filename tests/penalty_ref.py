"""The rule of include/qqq_amd_penalty.h restated in numpy, one token at a time in float32 / float16: a plain Python loop over every row,
every logits row of it and every distinct token of that row's sequence -- no scatter, no workspace, nothing of the kernel's algorithm.

    penalize(logits, ids, pos, seen, n_prompt, repetition, presence, frequency, vocab) -> (logits', seen')

logits float16 [rows * G, ld]; ids, pos int64 [rows] or [rows, G]; seen int32 [rows, seen_stride]; n_prompt int32 [rows]; the three
penalties float32 [rows] (or scalars).  The inputs are left as they are."""
from __future__ import annotations

import numpy as np


def rule(l16, c: int, rep, pres, freq):
    """One logit (np.float16) with c output occurrences -> np.float16; each line is one float32 operation."""
    rep, pres, freq = np.float32(rep), np.float32(pres), np.float32(freq)
    with np.errstate(all="ignore"):
        x = np.float32(l16)
        if rep != np.float32(1):
            x = np.float32(x / rep) if x > np.float32(0) else np.float32(x * rep)
        if c > 0:
            f = np.float32(freq * np.float32(c))
            x = np.float32(x - f)
            x = np.float32(x - pres)
        return np.float16(x)


def penalize(logits, ids, pos, seen, n_prompt, repetition, presence, frequency, vocab=None):
    logits = np.array(logits, dtype=np.float16, copy=True)
    seen = np.array(seen, dtype=np.int32, copy=True)
    ids = np.asarray(ids, dtype=np.int64)
    rows = ids.shape[0]
    ids = ids.reshape(rows, -1)
    pos = np.asarray(pos, dtype=np.int64).reshape(rows, -1)
    group = ids.shape[1]
    vocab = logits.shape[1] if vocab is None else int(vocab)
    assert logits.shape[0] == rows * group and seen.shape[0] == rows and vocab <= logits.shape[1]
    bc = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float32).reshape(-1), (rows,)) if np.ndim(v) else np.full(rows, v, np.float32)  # noqa: E731
    repetition, presence, frequency = bc(repetition), bc(presence), bc(frequency)
    for r in range(rows):
        p = int(pos[r, 0])
        if p < 0 or p >= seen.shape[1]:
            continue
        t0 = int(ids[r, 0])
        seen[r, p] = t0 if 0 <= t0 < vocab else -1
        rep, pres, freq = repetition[r], presence[r], frequency[r]
        if rep == np.float32(1) and pres == np.float32(0) and freq == np.float32(0):
            continue
        for j in range(group):
            seq = [int(t) for t in seen[r, :p + 1]] + [int(t) for t in ids[r, 1:j + 1]]
            outputs = {}
            for i, t in enumerate(seq):
                if 0 <= t < vocab:
                    outputs[t] = outputs.get(t, 0) + (1 if i >= int(n_prompt[r]) else 0)
            for t, c in outputs.items():
                logits[r * group + j, t] = rule(logits[r * group + j, t], c, rep, pres, freq)
    return logits, seen
