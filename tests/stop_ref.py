"""Plain-Python restatement of the per-row rules of qqq_ban_tokens and qqq_stop_check (include/qqq_amd_stop.h), written from
the header, on numpy arrays that are updated in place like the device's.  No vectorisation: one row, one end, one sequence at a time."""
import numpy as np

NEG_INF_BITS = np.uint16(0xFC00)


def ban_tokens(logits, n_out, min_new, eos, ban_ids=(), base=0, vocab=None):
    """logits: float16 [rows * G, ld], rewritten in place (columns vocab ... ld-1 are never touched) -> logits"""
    rows = len(n_out)
    total, ld = logits.shape
    vocab = ld if vocab is None else vocab
    group = total // rows if rows else 1
    bits = logits.view(np.uint16)
    for r in range(rows):
        for j in range(group):
            if int(n_out[r]) + base + j >= int(min_new[r]):
                continue
            for t in [int(eos[r])] + [int(b) for b in ban_ids]:
                if 0 <= t < vocab:
                    bits[r * group + j, t] = NEG_INF_BITS
    return logits


def completion_token(tokens, base, first, r, i):
    """c_r[i], or None where the index holds no token"""
    at = int(base[r]) + i
    if at < 0:
        return None if first is None else int(first[r])
    if at >= tokens.shape[1]:
        return None
    return int(tokens[r, at])


def stop_check(tokens, base, first, n_out, stop_ids, stop_len, min_new, n_seen, n_trim, stop_hit, ids, pos, slots, remaining, start=None,
               end_ids=(), eos=None):
    """every array a numpy array; n_seen, n_trim, stop_hit, ids, pos, slots, start and remaining are updated in place.  ids, pos and slots:
    [rows] or [rows, G]."""
    rows = len(n_out)
    n_stop = len(stop_len)
    for r in range(rows):
        m = int(n_out[r]) + 1
        a = max(int(n_seen[r]), 0)
        if a >= m:
            continue
        found = None
        for e in range(a + 1, m + 1):
            last = completion_token(tokens, base, first, r, e - 1)
            if eos is not None and int(eos[r]) >= 0 and last == int(eos[r]):
                found = (m - e, n_stop + len(end_ids))
                break
            for i, t in enumerate(end_ids):
                if int(t) >= 0 and last is not None and last == int(t):
                    found = (m - e, n_stop + i)
                    break
            if found is None and e >= int(min_new[r]):
                for s in range(n_stop):
                    L = int(stop_len[s])
                    if L < 1 or L > stop_ids.shape[1] or L > e:
                        continue
                    have = [completion_token(tokens, base, first, r, e - L + k) for k in range(L)]
                    if None not in have and have == [int(x) for x in stop_ids[s, :L]]:
                        found = (m - e + L, s)
                        break
            if found is not None:
                break
        if found is not None:
            n_trim[r], stop_hit[r] = found
            ids[r], pos[r], slots[r] = 0, -1, -1
            if start is not None:
                start[r] = -1
            remaining[r] = 0
        n_seen[r] = m
