"""What one generate() call asks for, checked once, and what every path that serves it does the same way.  The host loop of
QuantLlamaForCausalLM.generate (qqq_amd/model.py) and DecodeLoop.generate (qqq_amd/serve.py) keep the scheduling that is theirs and take
from a Request the checked keywords, the blocks a prompt's family needs, the keywords a loop is built and called with, sample() -- the
one pipeline from a pass's logits to its tokens --, receive() -- the one rule by which a completion ends -- and the shape of what the
call returns; Records collects the logprobs records.  Completions are numbered prompt * n + sibling throughout.  GuidedRequest is the
Request of generate_guided(): the same pipeline with ops.fsm_mask between the ban and the draw, and one automaton state per completion.
"""
from __future__ import annotations

from operator import index as _index
from typing import List, NamedTuple, Optional, Sequence

import torch

from . import ops


class TokenLogprobs(NamedTuple):
    """What generate(logprobs=k) returns per completion, one entry per emitted token (the eos included), as CPU tensors: the token's
    log-probability (f32 [T]) and rank (int32 [T], 1 = the most probable), and the k most probable tokens of its step with their
    log-probabilities (int32 / f32 [T, k]); see ops.topk_logprobs."""
    logprob: torch.Tensor
    rank: torch.Tensor
    top_ids: torch.Tensor
    top_logprobs: torch.Tensor

    @classmethod
    def empty(cls, k: int) -> "TokenLogprobs":
        return cls(torch.empty(0), torch.empty(0, dtype=torch.int32), torch.empty((0, k), dtype=torch.int32), torch.empty((0, k)))


def stop_arguments(name: str, vocab: int, stop, stop_token_ids, min_new_tokens):
    """generate()'s `stop`, `stop_token_ids` and `min_new_tokens`, checked -> (the stop sequences as lists, the stop ids, the minimum):
    at most 32 sequences of 1 ... 32 ids, at most 32 stop ids, every id in [0, vocab), a minimum >= 0.  `name` heads the messages."""
    def token(arg, t):
        try:
            t = None if isinstance(t, bool) else _index(t)
        except TypeError:
            t = None
        if t is None or not 0 <= t < vocab:
            raise ValueError(f"{name}: {arg} holds an entry that is no token id in [0, {vocab})")
        return t

    def rows(arg, value, what):
        # a sequence of any kind (a list, a tuple, an array, a tensor), None for none; a string or a scalar is not one
        if value is None:
            return []
        if isinstance(value, (str, bytes)):
            raise ValueError(f"{name}: {arg} must be {what}, not a string (encode stop strings first)")
        try:
            return list(value)
        except TypeError:
            raise ValueError(f"{name}: {arg} must be {what}") from None

    stops = [[token("stop", t) for t in rows("stop", s, "a sequence of token-id sequences")]
             for s in rows("stop", stop, "a sequence of token-id sequences")]
    if len(stops) > 32 or any(not 1 <= len(s) <= 32 for s in stops):
        raise ValueError(f"{name}: stop takes at most 32 sequences of 1 ... 32 token ids each")
    ids = [token("stop_token_ids", t) for t in rows("stop_token_ids", stop_token_ids, "a sequence of token ids")]
    if len(ids) > 32:
        raise ValueError(f"{name}: stop_token_ids takes at most 32 ids")
    try:
        least = -1 if isinstance(min_new_tokens, bool) else _index(min_new_tokens)
    except TypeError:
        least = -1
    if least < 0:
        raise ValueError(f"{name}: min_new_tokens={min_new_tokens!r} must be an int >= 0")
    return stops, ids, least


def stop_match(completion: Sequence[int], stops: Sequence[Sequence[int]]) -> int:
    """the length of the first stop sequence (lowest index) the completion ends in, 0 for none: include/qqq_amd_stop.h, rule 2"""
    for s in stops:
        if len(s) <= len(completion) and list(completion[len(completion) - len(s):]) == list(s):
            return len(s)
    return 0


def adapter_slots(name: str, lora, adapters, prompts: int) -> List[int]:
    """generate()'s `adapters` -- one slot of the bank `lora` or None per prompt; None: no prompt has one -- checked -> the slot per prompt,
    -1 for none.  `name` heads the messages."""
    if adapters is None:
        return [-1] * prompts
    if isinstance(adapters, (str, bytes)) or not hasattr(adapters, "__len__") or len(adapters) != prompts:
        raise ValueError(f"{name}: adapters must hold one entry per prompt ({prompts}): a slot of the bank, or None")
    slots = []
    for a in adapters:
        if a is not None:
            try:
                a = -1 if isinstance(a, bool) else _index(a)
            except TypeError:
                a = -1
            if not 0 <= a < lora.slots:
                raise ValueError(f"{name}: adapters holds an entry that is neither None nor a slot in [0, {lora.slots})")
        slots.append(-1 if a is None else a)
    return slots


class Records:
    """The logprobs=k records of one call: per pass the four device results of ops.topk_logprobs (k = 0 has no top-k parts), per completion
    its rows of them, in order, and `tail`: the four CPU parts a loop read back for its decode steps, which follow its first token's."""

    def __init__(self, k: int, completions: int):
        self.k, self.parts, self.rows, self.count, self.tail = k, ([], [], [], []), [[] for _ in range(completions)], 0, {}

    def add(self, parts, seqs: Sequence[int]) -> None:
        """a pass's results: row j of them is completion seqs[j]'s next record"""
        for kept, t in zip(self.parts, parts):
            if t is not None:
                kept.append(t)
        for row, q in enumerate(seqs):
            self.rows[q].append(self.count + row)
        self.count += len(seqs)

    def result(self, outs: Sequence[Sequence[int]]) -> List[TokenLogprobs]:
        """per completion its TokenLogprobs, cut like its tokens outs[q]; an empty one if it never drew.  The one transfer of the records."""
        if self.count:
            parts = [torch.cat(p).cpu() if p else torch.empty((self.count, 0), dtype=d) for p, d in
                     zip(self.parts, (torch.float32, torch.int32, torch.int32, torch.float32))]
        recs = []
        for q, at in enumerate(self.rows):
            rec = TokenLogprobs(*(p[torch.tensor(at)] for p in parts)) if at else TokenLogprobs.empty(self.k)
            if q in self.tail:
                rec = TokenLogprobs(*(torch.cat(pair) for pair in zip(rec, self.tail[q])))
            recs.append(TokenLogprobs(*(t[:len(outs[q])] for t in rec)))
        return recs


class Request:
    """The keywords of one generate() call, checked (`name` heads the messages: "generate", "DecodeLoop.generate", ...): temperature, top_k,
    top_p and generator as given; eos (-1: none); penalty (repetition, presence, frequency) and penalised; stops, end_ids and least
    (stop_arguments), stopping (one of the three is set) and ends, the tokens that end a completion and stay in it; n completions per
    prompt; k logprobs per record (None: no records); lora, the LoraBank of the call (None: no adapters, and then nothing of it runs) with
    `adapters`, one slot or None per prompt.  begin() adds the call's prompts, its completions `outs`, their `records` and `slots`, the
    prompts' adapter slots (-1: none)."""

    def __init__(self, name: str, vocab: int, temperature, top_k, top_p, generator, eos_token_id, repetition_penalty, presence_penalty,
                 frequency_penalty, stop, stop_token_ids, min_new_tokens, n, logprobs, lora=None, adapters=None):
        self.name, self.temperature, self.top_k, self.top_p, self.generator = name, temperature, top_k, top_p, generator
        self.n, self.k = n, logprobs  # checked where they are given: generate()'s keywords, a loop's family and logprobs
        self.penalty = (float(repetition_penalty), float(presence_penalty), float(frequency_penalty))
        if not (self.penalty[0] > 0.0 and self.penalty[0] != float("inf")):
            raise ValueError(f"{name}: repetition_penalty={self.penalty[0]} must be finite and > 0")
        self.penalised = self.penalty != (1.0, 0.0, 0.0)
        self.stops, self.end_ids, self.least = stop_arguments(name, vocab, stop, stop_token_ids, min_new_tokens)
        self.stopping = bool(self.stops or self.end_ids or self.least)
        self.eos = -1 if eos_token_id is None else int(eos_token_id)
        self.ends = set(self.end_ids) | ({self.eos} if self.eos >= 0 else set())
        self.lora, self.adapters = lora, adapters
        if lora is not None:
            from .lora import LoraBank

            if not isinstance(lora, LoraBank):
                raise ValueError(f"{name}: lora must be a LoraBank")
        elif adapters is not None:
            raise ValueError(f"{name}: adapters need lora, the LoraBank that holds them")

    def begin(self, prompts):
        """-> (the prompts as lists, the completions: n empty lists per prompt)"""
        self.prompts = [list(p) for p in prompts]
        if any(not p for p in self.prompts):
            raise ValueError(f"{self.name}: every prompt needs at least one token")
        self.outs: List[List[int]] = [[] for _ in range(len(self.prompts) * self.n)]
        self.records = Records(self.k, len(self.outs)) if self.k is not None else None
        self.slots = adapter_slots(self.name, self.lora, self.adapters, len(self.prompts))
        return self.prompts, self.outs

    def with_adapters(self, step, prompt_ids: Sequence[int], counts: Sequence[int]):
        """`step` (a PagedStep whose sequence j feeds counts[j] tokens of prompt prompt_ids[j]) with the tokens' adapter slots in
        step.lora -> step; untouched without a bank, and when no token of the step has an adapter"""
        if self.lora is not None:
            slots = [self.slots[i] for i, c in zip(prompt_ids, counts) for _ in range(c)]
            if any(s >= 0 for s in slots):
                step.lora = self.lora.step(self.lora.token_slots(slots))
        return step

    def family_blocks(self, prompt_len: int, keys: int, block_size: int) -> int:
        """the blocks a prompt's n completions of at most `keys` keys take: one budget plus, per further sibling, the blocks beyond the shared ones"""
        own = -(-keys // block_size)
        return own + (self.n - 1) * (own - prompt_len // block_size)

    def loop_keywords(self):
        """(what a loop that serves this request is built with, what its generate() takes besides): a keyword only when its feature is on"""
        build, call = {}, {}
        if self.n > 1:
            build["family"] = self.n
        if self.penalised:
            build["penalties"] = True
            call.update(zip(("repetition_penalty", "presence_penalty", "frequency_penalty"), self.penalty))
        if self.k is not None:
            build["logprobs"] = self.k
        if self.stopping:
            build["stops"] = True
            call.update(stop=self.stops, stop_token_ids=self.end_ids, min_new_tokens=self.least)
        if self.lora is not None:
            build["lora"] = self.lora
            call["adapters"] = self.adapters
        return build, call

    def sample(self, logits: torch.Tensor, seqs: Sequence[int], workspace: Optional[torch.Tensor]) -> torch.Tensor:
        """The tokens (int64 [len(seqs)], on the device) the completions `seqs` draw from a pass's `logits`: one row each, or -- the prefill
        of prompts with n > 1 -- one row per prompt, which serves the first draw of each of its siblings.  In this order, each only when
        its feature is on: ops.penalize_logits over prompts[q // n] + outs[q] (`workspace`: the op's); ops.ban_tokens at the counts
        len(outs[q]); one torch.rand(rows); ops.sample_tokens; ops.topk_logprobs into the records.  In a prefill pass outs[q] is empty."""
        if logits.shape[0] != len(seqs):
            logits = logits.repeat_interleave(self.n, dim=0)
        dev, n, prompts, outs = logits.device, self.n, self.prompts, self.outs
        if self.penalised:  # the history is host-side like the rest of the bookkeeping, padded per pass; its last token is the row's input
            hist = [prompts[q // n] + outs[q] for q in seqs]
            width = max(len(h) for h in hist)
            seen = torch.tensor([h + [-1] * (width - len(h)) for h in hist], dtype=torch.int32).to(dev)
            ops.penalize_logits(logits, torch.tensor([h[-1] for h in hist], dtype=torch.int64, device=dev),
                                torch.tensor([len(h) - 1 for h in hist], dtype=torch.int64, device=dev), seen,
                                torch.tensor([len(prompts[q // n]) for q in seqs], dtype=torch.int32, device=dev), *self.penalty, workspace)
        if self.least and any(len(outs[q]) < self.least for q in seqs):  # the host has the counts: a pass of rows at their minimum runs nothing
            r = len(seqs)  # one transfer: the rows' counts, minimum and eos and the stop ids (none: an empty view)
            packed = torch.tensor([len(outs[q]) for q in seqs] + [self.least] * r + [self.eos] * r + self.end_ids, dtype=torch.int32, device=dev)
            ops.ban_tokens(logits, *packed.split([r, r, r, len(self.end_ids)]), base=0)
        self._constrain(logits, seqs)
        u = torch.rand(logits.shape[0], generator=self.generator, device=dev)
        toks = ops.sample_tokens(logits, self.temperature, self.top_k, self.top_p, u)
        if self.records is not None:  # of the rows the sampler drew from; kept on the device until the call returns
            self.records.add(ops.topk_logprobs(logits, toks, self.k), seqs)
        return toks

    def _constrain(self, logits: torch.Tensor, seqs: Sequence[int]) -> None:
        """a subclass's last word on the rows the completions `seqs` draw from, behind the ban and in front of the draw: nothing here"""

    def receive(self, q: int, t: int, budget: int) -> bool:
        """completion q takes the token t it drew: whether it ends there -- on a token of `ends`, which stays; else, from `least` tokens
        on, on the first stop sequence it then ends in, cut in front of the match; else at `budget` tokens"""
        out = self.outs[q]
        out.append(t)
        if t in self.ends:
            return True
        cut = stop_match(out, self.stops) if len(out) >= self.least else 0
        self.cut(q, cut)
        return cut > 0 or len(out) >= budget

    def cut(self, q: int, count: int) -> None:
        """completion q drops its last `count` tokens (all, if it has fewer); result() cuts its records like it"""
        if count > 0:
            del self.outs[q][max(0, len(self.outs[q]) - count):]

    def result(self):
        """what the call returns: the completions, nested by prompt when n > 1, and with logprobs the records in the same nesting"""
        nest = lambda flat: flat if self.n == 1 else [flat[i:i + self.n] for i in range(0, len(flat), self.n)]  # noqa: E731
        return nest(self.outs) if self.records is None else (nest(self.outs), nest(self.records.result(self.outs)))


def merge_automata(name: str, fsm, prompts: int):
    """a guided call's `fsm` -- one TokenFSM for every prompt, or a sequence with one entry per prompt (None: unconstrained) -- checked
    -> (the merged automaton, the start state per prompt: TokenFSM.merge).  `name` heads the messages."""
    from .guided import TokenFSM

    given = [fsm] * prompts if fsm is None or isinstance(fsm, TokenFSM) else list(fsm)
    if len(given) != prompts:
        raise ValueError(f"{name}: fsm holds {len(given)} entries for {prompts} prompts (one TokenFSM, or one entry per prompt)")
    if any(f is not None and not isinstance(f, TokenFSM) for f in given):
        raise ValueError(f"{name}: fsm must be a TokenFSM, or a sequence of TokenFSM and None")
    return TokenFSM.merge(given)


class GuidedRequest(Request):
    """A Request whose completions follow token automata (qqq_amd/guided.py): `fsm` is one TokenFSM for every prompt or a sequence with one
    entry per prompt (None: that prompt is unconstrained).  begin() merges them and gives every completion its start state; `state` holds
    one host state per completion: -1 for no automaton, -2 once a token outside the automaton was drawn.  sample() masks the rows by
    those states (ops.fsm_mask, behind the penalties and the ban), receive() steps them by the rules of
    include/qqq_amd_guided.h and ends a completion that reaches a terminal state; a loop writes the states its rows ended in back into `state`."""

    def __init__(self, fsm, *args, **kw):
        super().__init__(*args, **kw)
        self._given = fsm

    def begin(self, prompts):
        prompts, outs = super().begin(prompts)
        self.fsm, starts = merge_automata(self.name, self._given, len(prompts))
        self.state = [s for s in starts for _ in range(self.n)]
        return prompts, outs

    def _constrain(self, logits: torch.Tensor, seqs: Sequence[int]) -> None:
        packed = torch.tensor([self.state[q] for q in seqs] + [self.eos] * len(seqs), dtype=torch.int32, device=logits.device)
        state, eos = packed.split([len(seqs), len(seqs)])
        ops.fsm_mask(logits, state, self.fsm.tensors(logits.device), eos=eos)

    def receive(self, q: int, t: int, budget: int) -> bool:
        s, ended = self.state[q], super().receive(q, t, budget)
        if not 0 <= s < self.fsm.n_states:
            return ended
        to = self.fsm.step(s, t)
        if to < 0 and self.fsm.accept[s] and t == self.eos >= 0:
            return ended  # the eos in an accepting state: the state stays
        self.state[q] = to
        return ended or to < 0 or self.fsm.terminal(to)

    def check(self) -> None:
        """raises if a completion drew a token outside its automaton (state -2)"""
        bad = [q for q, s in enumerate(self.state) if s == -2]
        if bad:
            raise RuntimeError(f"{self.name}: completion {bad[0]} (of {len(bad)}) drew a token outside its automaton: every token its state "
                               f"allows had a logit of -inf or NaN")


__all__ = ["adapter_slots", "GuidedRequest", "merge_automata", "Request", "Records", "TokenLogprobs", "stop_arguments", "stop_match"]
