"""Guided decoding: a deterministic automaton over token ids that says which tokens a completion may draw next
(include/qqq_amd_guided.h).  Pure Python and numpy; ops.fsm_mask / ops.fsm_advance walk the same arrays on the device, GuidedRequest
(qqq_amd/request.py) on the host.

    TokenFSM(offsets, tokens, next, accept, start)   the automaton in CSR form, validated
    TokenFSM.from_choices / from_allowed / from_dfa  "one of these token sequences", "only these ids", "whatever this byte-level DFA takes"
    TokenFSM.merge                                   a disjoint union, so that the prompts of one call follow different automata

There is no tokenizer and no regex or JSON-schema compiler here: callers bring token ids, or a byte-level DFA and their vocabulary's bytes.
"""
from __future__ import annotations

from operator import index as _index
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

NO_EDGE = -2  # the state of a completion that drew a token outside its automaton
IDLE = -1     # the state of a row or prompt that follows no automaton


class TokenFSM:
    """A deterministic automaton over token ids, states 0 ... S - 1, in CSR form:

        offsets  int32 [S + 1]  non-decreasing, offsets[0] = 0, offsets[S] = E: state s owns the edges offsets[s] ... offsets[s + 1] - 1
        tokens   int32 [E]      an edge's token, strictly ascending inside each state, every one in [0, vocab)
        next     int32 [E]      an edge's target state, in [0, S)
        accept   int32 [S]      non-zero: the row's eos may be drawn in this state
        start    int            the initial state
        vocab    int or None    the bound of the token ids (None: only >= 0 is checked)

    A state without edges is TERMINAL: reaching it completes the completion, and no eos is drawn.  The constructor checks every
    property above, in that order, and raises ValueError naming the first one violated."""

    def __init__(self, offsets, tokens, next, accept, start: int = 0, vocab: Optional[int] = None):  # noqa: A002
        def array(name, a):
            a = np.asarray(a)
            if a.dtype == object or a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)) or a.dtype == np.bool_:
                raise ValueError(f"TokenFSM: {name} must be a one-dimensional array of integers")
            if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise ValueError(f"TokenFSM: {name} holds a value outside int32")
            return np.ascontiguousarray(a, dtype=np.int32)

        offsets, tokens, nxt, accept = (array(n, a) for n, a in (("offsets", offsets), ("tokens", tokens), ("next", next), ("accept", accept)))
        S, E = accept.shape[0], tokens.shape[0]
        if S < 1:
            raise ValueError("TokenFSM: accept must hold at least one state")
        if offsets.shape[0] != S + 1:
            raise ValueError(f"TokenFSM: offsets must hold S + 1 = {S + 1} entries, not {offsets.shape[0]}")
        if offsets[0] != 0:
            raise ValueError(f"TokenFSM: offsets[0] = {offsets[0]} must be 0")
        if np.any(np.diff(offsets) < 0):
            raise ValueError("TokenFSM: offsets must be non-decreasing")
        if offsets[S] != E:
            raise ValueError(f"TokenFSM: offsets[S] = {offsets[S]} must be the number of edges E = {E}")
        if nxt.shape[0] != E:
            raise ValueError(f"TokenFSM: next must hold E = {E} entries like tokens, not {nxt.shape[0]}")
        if vocab is not None:
            vocab = _index(vocab)
            if vocab < 1:
                raise ValueError(f"TokenFSM: vocab={vocab} must be at least 1")
        if E and (tokens.min() < 0 or (vocab is not None and tokens.max() >= vocab)):
            raise ValueError(f"TokenFSM: tokens holds an id outside [0, {'2^31' if vocab is None else vocab})")
        if E > 1:
            inner = np.ones(E, dtype=bool)  # an edge that is not the first of its state
            inner[offsets[:-1][offsets[:-1] < E]] = False
            if np.any((np.diff(tokens) <= 0) & inner[1:]):
                raise ValueError("TokenFSM: tokens must be strictly ascending inside each state")
        if E and (nxt.min() < 0 or nxt.max() >= S):
            raise ValueError(f"TokenFSM: next holds a state outside [0, {S})")
        start = _index(start)
        if not 0 <= start < S:
            raise ValueError(f"TokenFSM: start={start} outside [0, {S})")
        self.offsets, self.tokens, self.next, self.accept, self.start, self.vocab = offsets, tokens, nxt, accept, start, vocab
        self._tensors: Dict[str, tuple] = {}

    # ---- what it holds

    @property
    def n_states(self) -> int:
        return self.accept.shape[0]

    @property
    def n_edges(self) -> int:
        return self.tokens.shape[0]

    def terminal(self, s: int) -> bool:
        return 0 <= s < self.n_states and self.offsets[s] == self.offsets[s + 1]

    def allowed(self, s: int) -> List[int]:
        """the tokens with an edge out of state s, ascending (a state outside [0, S): none)"""
        if not 0 <= s < self.n_states:
            return []
        return self.tokens[self.offsets[s]:self.offsets[s + 1]].tolist()

    def step(self, s: int, t: int) -> int:
        """the state behind token t in state s: NO_EDGE (-2) where there is no edge; a state outside [0, S) stays what it is"""
        if not 0 <= s < self.n_states:
            return s
        lo, hi = int(self.offsets[s]), int(self.offsets[s + 1])
        at = lo + int(np.searchsorted(self.tokens[lo:hi], t))
        return int(self.next[at]) if at < hi and self.tokens[at] == t else NO_EDGE

    def walk(self, tokens: Sequence[int], eos: Optional[int] = None, start: Optional[int] = None) -> int:
        """the state behind `tokens` from `start` by the device's rules (include/qqq_amd_guided.h): a token without an edge that
        is `eos` in an accepting state leaves the state as it is, any other gives NO_EDGE"""
        s = self.start if start is None else start
        for t in tokens:
            if not 0 <= s < self.n_states:
                break
            to = self.step(s, t)
            if to == NO_EDGE and eos is not None and eos >= 0 and t == eos and self.accept[s]:
                continue
            s = to
        return s

    def accepts(self, tokens: Sequence[int], eos: Optional[int] = None, start: Optional[int] = None) -> bool:
        """whether `tokens` is a whole completion of the automaton: every token has an edge (a last `eos` drawn in an accepting state
        aside), nothing follows a terminal state or the eos, and the walk ends in an accepting or a terminal state"""
        s = self.start if start is None else start
        tokens = list(tokens)
        for j, t in enumerate(tokens):
            if self.terminal(s):
                return False
            to = self.step(s, t)
            if to == NO_EDGE:
                return bool(eos is not None and eos >= 0 and t == eos and self.accept[s] and j == len(tokens) - 1)
            s = to
        return 0 <= s < self.n_states and bool(self.accept[s] or self.terminal(s))

    def tensors(self, device):
        """(offsets, tokens, next, accept) as int32 tensors on `device`, made once per device"""
        import torch

        key = str(torch.device(device))
        if key not in self._tensors:
            self._tensors[key] = tuple(torch.from_numpy(a.copy()).to(device) for a in (self.offsets, self.tokens, self.next, self.accept))
        return self._tensors[key]

    # ---- builders

    @classmethod
    def _from_edges(cls, edges: List[Dict[int, int]], accept: Sequence[int], start: int, vocab: Optional[int]) -> "TokenFSM":
        """edges[s] = {token: target}"""
        counts = [len(e) for e in edges]
        offsets = np.zeros(len(edges) + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        tokens = np.fromiter((t for e in edges for t in sorted(e)), dtype=np.int64, count=int(offsets[-1]))
        nxt = np.fromiter((e[t] for e in edges for t in sorted(e)), dtype=np.int64, count=int(offsets[-1]))
        return cls(offsets, tokens, nxt, np.asarray(accept, dtype=np.int64), start, vocab)

    @classmethod
    def from_choices(cls, choices: Sequence[Sequence[int]], vocab: Optional[int] = None) -> "TokenFSM":
        """The completion is one of `choices` (token-id sequences; duplicates are one choice): a trie.  The end of a choice that no other
        choice extends is a terminal state; the end of a choice that is a proper prefix of another is an accepting state that keeps its
        edges (the row's eos ends the completion there).  An empty choice makes the start state accepting."""
        choices = [[_index(t) for t in c] for c in choices]
        if not choices:
            raise ValueError("TokenFSM.from_choices: at least one choice is needed")
        edges: List[Dict[int, int]] = [{}]
        accept = [0]
        for c in choices:
            s = 0
            for t in c:
                if t not in edges[s]:
                    edges[s][t] = len(edges)
                    edges.append({})
                    accept.append(0)
                s = edges[s][t]
            accept[s] = 1
        return cls._from_edges(edges, accept, 0, vocab)

    @classmethod
    def from_allowed(cls, ids: Sequence[int], vocab: Optional[int] = None) -> "TokenFSM":
        """Only the token ids `ids` (vLLM's allowed_token_ids): one accepting state with a self-loop per id."""
        ids = sorted({_index(t) for t in ids})
        if not ids:
            raise ValueError("TokenFSM.from_allowed: at least one id is needed")
        return cls([0, len(ids)], ids, [0] * len(ids), [1], 0, vocab)

    @classmethod
    def from_dfa(cls, transitions: Dict[int, Dict[int, int]], start: int, finals: Sequence[int], vocab: Sequence[bytes]) -> "TokenFSM":
        """The token-level index of a byte-level DFA `transitions` = {state: {byte: state}} with start state `start` and final states
        `finals`: token id i stands for the bytes vocab[i] (an empty entry is never allowed), and has an edge out of a state where all its
        bytes walk the DFA.  States from which no final state can be reached are dropped with the edges into them, so a guided run never
        dead-ends; states no token path reaches are dropped too.  A final state is accepting; one without token edges is terminal.
        The walk is vectorised over the vocabulary: one numpy gather per byte position, over all states at once."""
        names = sorted(set(transitions) | {start} | set(finals) | {to for row in transitions.values() for to in row.values()})
        number = {q: i for i, q in enumerate(names)}
        Q, V = len(names), len(vocab)
        if V < 1:
            raise ValueError("TokenFSM.from_dfa: the vocabulary is empty")
        table = np.full((Q + 1, 256), Q, dtype=np.int32)  # row Q: the dead state
        for q, row in transitions.items():
            for b, to in row.items():
                table[number[q], b[0] if isinstance(b, (bytes, bytearray)) else int(b)] = number[to]
        width = max((len(w) for w in vocab), default=0)
        length = np.fromiter((len(w) for w in vocab), dtype=np.int64, count=V)
        text = np.zeros((V, max(width, 1)), dtype=np.uint8)
        for i, w in enumerate(vocab):
            text[i, :len(w)] = np.frombuffer(bytes(w), dtype=np.uint8)
        at = np.repeat(np.arange(Q, dtype=np.int32)[:, None], V, axis=1)  # [Q, V]: where token v stands, begun in state q
        for j in range(width):
            live = length > j
            at[:, live] = table[at[:, live], text[live, j][None, :]]
        at[:, length == 0] = Q
        final = np.zeros(Q + 1, dtype=bool)
        final[[number[q] for q in finals]] = True
        # trim: the states that reach a final one over token edges (backwards), among them the ones the start reaches (forwards)
        src, tok = np.nonzero(at < Q)
        dst = at[src, tok]
        good = final[:Q].copy()
        while True:
            more = good.copy()
            more[src[good[dst]]] = True
            if (more == good).all():
                break
            good = more
        if not good[number[start]]:
            raise ValueError("TokenFSM.from_dfa: no sequence of tokens takes the start state to a final one")
        keep = good[src] & good[dst]
        src, tok, dst = src[keep], tok[keep], dst[keep]
        seen = np.zeros(Q, dtype=bool)
        seen[number[start]] = True
        while True:
            more = seen.copy()
            more[dst[seen[src]]] = True
            if (more == seen).all():
                break
            seen = more
        keep = seen[src]
        src, tok, dst = src[keep], tok[keep], dst[keep]
        new = np.cumsum(seen) - 1  # np.nonzero gave (state, token) in ascending order: the edges are sorted as they stand
        S = int(seen.sum())
        offsets = np.zeros(S + 1, dtype=np.int64)
        np.cumsum(np.bincount(new[src], minlength=S), out=offsets[1:])
        return cls(offsets, tok, new[dst], final[:Q][seen].astype(np.int32), int(new[number[start]]), V)

    @staticmethod
    def merge(fsms: Sequence[Optional["TokenFSM"]]) -> Tuple["TokenFSM", List[int]]:
        """(the disjoint union of `fsms` with renumbered states, the start state of each): a None entry -- no automaton -- gives start -1.
        An automaton given several times (the same object) is taken once.  With nothing but None: one accepting state without edges."""
        parts: List[TokenFSM] = []
        base: Dict[int, int] = {}
        starts, states, edges = [], 0, 0
        for f in fsms:
            if f is None:
                starts.append(IDLE)
                continue
            if not isinstance(f, TokenFSM):
                raise ValueError("TokenFSM.merge: every entry must be a TokenFSM or None")
            if id(f) not in base:
                base[id(f)] = states
                parts.append(f)
                states += f.n_states
                edges += f.n_edges
            starts.append(base[id(f)] + f.start)
        if not parts:
            return TokenFSM([0, 0], [], [], [1], 0), starts
        if len(parts) == 1:
            return parts[0], starts
        vocabs = [f.vocab for f in parts]
        off, at_s, at_e = [np.zeros(1, dtype=np.int64)], 0, 0
        nxt = []
        for f in parts:
            off.append(f.offsets[1:].astype(np.int64) + at_e)
            nxt.append(f.next.astype(np.int64) + at_s)
            at_s, at_e = at_s + f.n_states, at_e + f.n_edges
        merged = TokenFSM(np.concatenate(off), np.concatenate([f.tokens for f in parts]), np.concatenate(nxt),
                          np.concatenate([f.accept for f in parts]), 0, None if None in vocabs else max(vocabs))
        return merged, starts


__all__ = ["TokenFSM", "NO_EDGE", "IDLE"]
