"""The device-resident decode loop: a fixed number of rows whose per-step metadata lives in device memory and is advanced there by
ops.sample_advance, so that one decode step -- model forward + sample_advance -- reads nothing on the host and is ONE captured graph,
replayed `sync_every` times between host syncs while rows finish and join without re-capture.

    DecodeLoop      the rows' state arrays (include/qqq_amd_step.h), the one PagedStep built over them, the captured step, and generate()
    SpecDecodeLoop  the same loop with draft_len guessed tokens behind every row's last one, verified on the device by ops.spec_advance
                    (include/qqq_amd_spec.h): a replay emits 1 ... draft_len + 1 tokens per row.  Opt-in.
    GuidedDecodeLoop  DecodeLoop whose rows follow token automata held in device memory (qqq_amd/guided.py): ops.fsm_mask in front of the
                    sampler and ops.fsm_advance behind it, through DecodeLoop's _before_sample / _after_sample hooks.  Opt-in.
    ngram_draft     the drafter's rule in plain Python: what the device computes from a row's history, and what the host writes at admission

QuantLlamaForCausalLM.generate (qqq_amd/model.py) builds its batch anew on the host for every token: a PagedKVCache.step, an eager launch
of every kernel, a tolist() before the next step.  Here the host only admits prompts (an eager packed prefill, the first token from
ops.sample_tokens), writes the admitted rows' state with indexed copies, replays, and reads (n_out, remaining) back once per `sync_every`
steps.  A row that is idle (pos -1, slot -1, remaining 0) rides along in every step and is inert: see include/qqq_amd_step.h.

generate() -- admission, prefill, the run / sync / retire loop and the cleanup -- exists once, on DecodeLoop; the checks of its keywords,
an admitted prompt's first token, the rule by which a completion ends and the shape of the result are the Request's (qqq_amd/request.py),
as in QuantLlamaForCausalLM.generate.  SpecDecodeLoop inherits it and overrides _decode_step, _run, _start_call, _budget_words, _row_state,
_penalty_state, _stop_state, _stop_check and _collect, and the attributes _tokens, _synced and _idle.
"""
from __future__ import annotations

from collections import deque
from typing import List, Optional, Sequence

import torch

from . import ops
from .paged import PagedKVCache, PagedStep
from .request import GuidedRequest, Request, merge_automata


def _check_loop(name, lm, cache, rows, max_len, sync_every, graph, u_stride_error=None):
    """The checks every loop makes on its construction arguments, in this order -> the model's device.  `u_stride_error`: what the
    loop's own check of u_stride found, or None."""
    if not isinstance(cache, PagedKVCache):
        raise TypeError(f"{name}: cache must be a PagedKVCache")
    if rows < 1 or rows > 65535 or max_len < 1 or sync_every < 1:
        raise ValueError(f"{name}: rows={rows}, max_len={max_len} and sync_every={sync_every} must be at least 1 (rows <= 65535)")
    if u_stride_error:
        raise ValueError(f"{name}: {u_stride_error}")
    if max_len > cache.capacity:
        raise ValueError(f"{name}: max_len={max_len} exceeds what the pool could hold ({cache.capacity} keys)")
    dev = lm.lm_head.weight.device
    if cache.k[0].device != dev:
        raise RuntimeError(f"{name}: the model and the cache must be on the same device")
    if graph and dev.type != "cuda":
        raise RuntimeError(f"{name}: graph=True needs the model on the GPU (and the ops of a step have no CPU path)")
    return dev


class DecodeLoop:
    """`rows` decode rows over `cache` for sequences of at most `max_len` keys (prompt and generated tokens but the last).

    lm          a QuantLlamaForCausalLM on the GPU;  cache  a PagedKVCache of its shape (it may hold other sequences)
    rows        the batch of every decode step, idle rows included; fixed, as is max_len: the decode kernel's split plan is a function of
                (rows, kv heads, max_len), so a captured step holds for exactly these two
    sync_every  decode steps between two host syncs;  u_stride  uniform variates per row and refill (>= sync_every)
    graph       True: the step is captured once into a torch.cuda.CUDAGraph (on a side stream; single-stream, straight-line) and replayed;
                False: the same calls run eagerly.  Both give the same tokens.
    penalties   True: the loop owns what ops.penalize_logits takes -- `seen` (int32 [rows, max_len], the rows' prompts and emitted tokens),
                n_prompt, repetition, presence, frequency and the op's workspace -- and its step runs that op between the forward and the
                sampler, inside the captured graph; generate() then takes repetition_penalty, presence_penalty and frequency_penalty.
                A row whose three values are 1, 0 and 0 rides through it with its logits untouched.  False: none of that exists.
    family      N > 1 (parallel sampling): rows [k * N, (k + 1) * N) are a fixed slot for the N completions of one prompt, rows % N == 0.  The
                loop then owns `family_of` (int32 [rows], constant: a row's slot's first row) and `shared` (int64 [rows]: the keys a row has
                in common with its siblings, written on admission, 0 when idle) inside its PagedStep, as part of the captured graph: a model
                with fuse_shared() reads a family's common keys once per pack of rows.  generate() then returns N lists per prompt.
    logprobs    k in [0, 32] (None: off): the loop owns `n_rec` (int32 [rows]: the records a row has), `lp` / `lp_rank` (f32 / int32
                [rows, max_len]) and `lp_top_ids` / `lp_top` (int32 / f32 [rows, max_len, k]), and its step runs ops.topk_logprobs_step
                behind ops.sample_advance, inside the captured graph: every emitted token's log-probability, rank and k most probable
                alternatives, from the logits row it was drawn from.  generate() then returns (tokens, records).  None: none of that exists.
    stops       True: the loop owns what ops.ban_tokens and ops.stop_check take (include/qqq_amd_stop.h) -- min_new, n_seen,
                n_trim, stop_hit, stop_base and first (int32 [rows]), the table stop_ids / stop_len (int32 [32, 32] / [32]) and the stop
                token ids ban_ids (int32 [32], -1 = unused) -- and its step runs the ban between the penalties and the sampler and the
                check behind the sampler (and the records), inside the captured graph; generate() then takes stop, stop_token_ids and
                min_new_tokens.  The tables have fixed shapes, so one capture serves every call.  False: none of that exists.
    lora        a LoraBank (qqq_amd/lora.py; None: off): the loop owns `lora_slot` (int32 [rows]: a row's adapter slot, written on admission,
                -1 for none and when idle) inside its PagedStep, as part of the captured graph: every targeted projection of the step is
                followed by ops.lora_add, which reads the slots on the device; generate() then takes adapters, one slot or None per prompt.
                One capture serves every mix of adapters, and the bank's load() / unload() between calls.  None: none of that exists.
    `captures` counts the captures: 1 for the life of the loop with graph=True.  The graph holds addresses: a model that is changed after
    the first generate() (fuse_*(), load_state_dict, .to()) needs a new loop."""

    _name = "DecodeLoop"
    group = 1                        # tokens a row feeds through a step, and variates it uses
    _tokens = "out"                  # the array a finished row's tokens are read from
    _synced = ("n_out", "remaining")  # what a sync transfers
    _idle = (("remaining", 0), ("pos", -1), ("slots", -1), ("ids", 0))  # what the cleanup resets
    family = 1                       # rows per slot: the completions of one prompt (DecodeLoop alone takes more than 1)
    penalties = False                # True: the step runs ops.penalize_logits in front of the sampler (_allocate_penalties)
    logprobs = None                  # k: the step runs ops.topk_logprobs_step behind the sampler (DecodeLoop alone takes it)
    stops = False                    # True: the step runs ops.ban_tokens in front of the sampler and ops.stop_check behind it (_allocate_stops)
    lora = None                      # a LoraBank: the step's projections are followed by ops.lora_add over `lora_slot` (_allocate_lora)

    def __init__(self, lm, cache: PagedKVCache, rows: int, max_len: int, sync_every: int = 8, u_stride: int = 64, graph: bool = True,
                 penalties: bool = False, family: int = 1, logprobs: Optional[int] = None, lora=None, stops: bool = False):
        rows, max_len, sync_every, u_stride, family = int(rows), int(max_len), int(sync_every), int(u_stride), int(family)
        short = u_stride < sync_every and f"u_stride={u_stride} must cover the sync_every={sync_every} steps between two refills"
        dev = _check_loop("DecodeLoop", lm, cache, rows, max_len, sync_every, graph, short)
        if family < 1 or rows % family:
            raise ValueError(f"DecodeLoop: family={family} must be at least 1 and divide rows={rows}")
        if logprobs is not None and not 0 <= int(logprobs) <= min(32, lm.lm_head.weight.shape[0]):
            raise ValueError(f"DecodeLoop: logprobs={logprobs} outside [0, min(32, vocab)]")
        self.family = family
        self._allocate(lm, cache, rows, max_len, sync_every, u_stride, graph, dev)
        self.out = torch.zeros((rows, max_len), dtype=torch.int64, device=dev)
        if logprobs is not None:  # one record per emitted token: out's shape
            self.logprobs = int(logprobs)
            self.n_rec = torch.zeros(rows, dtype=torch.int32, device=dev)
            self.lp = torch.zeros((rows, max_len), dtype=torch.float32, device=dev)
            self.lp_rank = torch.zeros((rows, max_len), dtype=torch.int32, device=dev)
            self.lp_top_ids = torch.zeros((rows, max_len, self.logprobs), dtype=torch.int32, device=dev)
            self.lp_top = torch.zeros((rows, max_len, self.logprobs), dtype=torch.float32, device=dev)
        if penalties:  # this loop keeps no history of its own: the penalty op records a row's input token at its position
            self._allocate_penalties(torch.zeros((rows, max_len), dtype=torch.int32, device=dev))
        if stops:  # the completion is the prefill's token and then `out`: index -1 of out is `first`
            self._allocate_stops(-1)
            self.first = torch.zeros(rows, dtype=torch.int32, device=dev)
        # the one step of every decode pass: its device tensors ARE the state arrays (a row's position is its last position)
        self.step = PagedStep(seq_ids=[None] * rows, counts=[1] * rows, starts=[0] * rows, max_len=max_len, decode=True, pos=self.pos,
                              slots=self.slots, block_table=self.block_table, last_pos=self.pos,
                              cu_tokens=torch.arange(rows + 1, dtype=torch.int32, device=dev), start_pos=self.pos)
        if family > 1:  # the slots are fixed: what changes from prompt to prompt is `shared`
            self.family_of = (torch.arange(rows, dtype=torch.int32, device=dev) // family) * family
            self.shared = torch.zeros(rows, dtype=torch.int64, device=dev)
            self.step.family, self.step.shared, self.step.family_max = self.family_of, self.shared, family
        if lora is not None:
            self._allocate_lora(lora)

    def _allocate_lora(self, bank) -> None:
        """What a loop built with lora=bank owns: `lora_slot`, one adapter slot per token of the step (a row's slot repeated over its
        chunk), every row idle (-1), held by the step the graph captures."""
        if bank.device != self.device:
            raise RuntimeError(f"{self._name}: the bank and the model must be on the same device")
        self.lora = bank
        self.lora_slot = torch.full((self.rows,) if self.group == 1 else (self.rows, self.group), -1, dtype=torch.int32, device=self.device)
        self.step.lora = bank.step(self.lora_slot.view(-1))

    def _allocate(self, lm, cache, rows, max_len, sync_every, u_stride, graph, dev):
        """The attributes and state arrays every loop has, for rows of `self.group` tokens: [rows] at 1, [rows, group] beyond."""
        self.lm, self.cache, self.rows, self.max_len, self.sync_every, self.u_stride = lm, cache, rows, max_len, sync_every, u_stride
        self.graph, self.device, self.captures = bool(graph), dev, 0
        per_token = (rows,) if self.group == 1 else (rows, self.group)
        i32 = dict(dtype=torch.int32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.ids = torch.zeros(per_token, **i64)
        self.pos = torch.full(per_token, -1, **i64)
        self.slots = torch.full(per_token, -1, **i64)
        self.block_table = torch.zeros((rows, -(-max_len // cache.block_size)), **i32)
        self.remaining = torch.zeros(rows, **i32)
        self.eos = torch.full((rows,), -1, **i32)
        self.n_out = torch.zeros(rows, **i32)
        self.tick = torch.zeros(rows, **i32)
        self.u = torch.zeros((rows, u_stride), **f32)
        self.temperature = torch.zeros(rows * self.group, **f32)  # the sampler's parameters: one per logits row
        self.top_k = torch.zeros(rows * self.group, **i32)
        self.top_p = torch.ones(rows * self.group, **f32)
        self._graph = None
        self._used = u_stride  # variates of u consumed since its last refill: none are left

    def _allocate_penalties(self, seen: torch.Tensor) -> None:
        """What ops.penalize_logits takes beside ids and pos, for a loop built with penalties=True: `seen` is the rows' history (of
        prompt and emitted tokens, int32 [rows, max_len]); every row starts neutral (1, 0, 0)."""
        i32 = dict(dtype=torch.int32, device=self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.penalties, self.seen = True, seen
        self.n_prompt = torch.zeros(self.rows, **i32)
        self.repetition = torch.ones(self.rows, **f32)
        self.presence = torch.zeros(self.rows, **f32)
        self.frequency = torch.zeros(self.rows, **f32)
        self.penalty_workspace = torch.zeros(self.rows * self.lm.lm_head.weight.shape[0], **i32)  # zero between any two calls

    def _allocate_stops(self, base: int) -> None:
        """What ops.ban_tokens and ops.stop_check take, for a loop built with stops=True: every row idle and checked (n_seen = n_out + 1),
        no stop sequence, no stop id, no minimum.  `base`: where a row's completion begins in its line of the `_tokens` array."""
        i32 = dict(dtype=torch.int32, device=self.device)
        self.stops = True
        self.min_new = torch.zeros(self.rows, **i32)
        self.n_seen = torch.ones(self.rows, **i32)
        self.n_trim = torch.zeros(self.rows, **i32)
        self.stop_hit = torch.full((self.rows,), -1, **i32)
        self.stop_base = torch.full((self.rows,), base, **i32)
        self.stop_ids = torch.zeros((32, 32), **i32)
        self.stop_len = torch.zeros(32, **i32)
        self.ban_ids = torch.full((32,), -1, **i32)

    def _ban(self, logits: torch.Tensor) -> None:
        ops.ban_tokens(logits, self.n_out, self.min_new, self.eos, self.ban_ids, base=1)  # n_out does not count the prefill's token

    def _stop_check(self) -> None:
        ops.stop_check(self.out, self.stop_base, self.first, self.n_out, self.stop_ids, self.stop_len, self.min_new, self.n_seen,
                       self.n_trim, self.stop_hit, self.ids, self.pos, self.slots, self.remaining, end_ids=self.ban_ids, eos=self.eos)

    def _penalize(self, logits: torch.Tensor) -> None:
        ops.penalize_logits(logits, self.ids, self.pos, self.seen, self.n_prompt, self.repetition, self.presence, self.frequency,
                            self.penalty_workspace)

    # ---- one decode step

    def _decode_step(self) -> None:
        logits = self.lm(self.ids, self.cache, self.step)
        if self.penalties:
            self._penalize(logits)
        if self.stops:
            self._ban(logits)
        self._before_sample(logits)
        ops.sample_advance(logits, self.temperature, self.top_k, self.top_p, self.u, self.tick, self.ids, self.pos, self.slots,
                           self.block_table, self.remaining, self.eos, self.out, self.n_out, self.cache.block_size)
        if self.logprobs is not None:  # the row that just emitted a token has n_rec < n_out: its record, from the logits it was drawn from
            ops.topk_logprobs_step(logits, self.out, self.n_out, self.n_rec, self.lp, self.lp_rank, self.lp_top_ids, self.lp_top)
        if self.stops:  # a row that eos or the budget just retired is checked too: its n_seen is behind its n_out
            self._stop_check()
        self._after_sample(logits)

    def _before_sample(self, logits: torch.Tensor) -> None:
        """a subclass's last word on the step's logits, behind the penalties and the ban: nothing here"""

    def _after_sample(self, logits: torch.Tensor) -> None:
        """a subclass's epilogue of the step, behind the sampler, the records and the stop check: nothing here"""

    def _capture(self) -> None:
        """Warm up and capture the step with every row idle (nothing but `tick` changes), on a side stream."""
        if bool((self.remaining != 0).any()):
            raise RuntimeError(f"{self._name}: the step is captured with every row idle")
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            self._decode_step()  # outside the capture: rope tables, GEMM workspaces and the allocator's pools come to exist here
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                self._decode_step()
        torch.cuda.current_stream(self.device).wait_stream(side)
        self.tick.zero_()
        # the graph holds addresses: the rope tables it read stay alive with it, even if a longer sequence elsewhere regrows the modules'
        self._tables = [(m._cos, m._sin) for m in self.lm.modules() if getattr(m, "_cos", None) is not None]
        self._graph = graph
        self.captures += 1

    def _run(self, steps: int, generator) -> None:
        if self._used + steps * self.group > self.u_stride:  # tick is about to wrap: new variates, and the rows start over at the first
            self.u.copy_(torch.rand((self.rows, self.u_stride), generator=generator, device=self.device))
            self.tick.zero_()
            self._used = 0
        self._used += steps * self.group
        for _ in range(steps):
            if self._graph is not None:
                self._graph.replay()
            else:
                self._decode_step()

    # ---- what differs between the loops

    def _start_call(self) -> None:
        self._used = self.u_stride  # this call draws with its own generator alone: nothing an earlier call left in u is used

    def _budget_words(self, new: int):
        """(the keys a sequence needs beyond its prompt and its new tokens but the last, how the two budget messages name the parts)"""
        return 0, f" and {new} new ones", "prompt and budget"

    def _row_state(self, prompt: List[int], first: int, blocks: List[int]) -> dict:
        """What an admitted row writes, per state array: `prompt` is in the cache, `first` the token the prefill drew."""
        p, bs = len(prompt), self.cache.block_size
        table = blocks + [0] * (self.block_table.shape[1] - len(blocks))
        penalty = self._penalty_state(prompt) if self.penalties else {}
        stop = self._stop_state(prompt, first) if self.stops else {}
        return dict(ids=first, pos=p, slots=blocks[p // bs] * bs + p % bs, block_table=table, **penalty, **stop)

    def _penalty_state(self, prompt: List[int]) -> dict:
        """What an admitted row of a loop with penalties writes besides: the prompt is what the row has seen (the op records the rest)."""
        return dict(n_prompt=len(prompt), seen=prompt + [0] * (self.seen.shape[1] - len(prompt)))

    def _stop_state(self, prompt: List[int], first: int) -> dict:
        """What an admitted row of a loop with stops writes besides: how ops.stop_check finds the completion's first token."""
        return dict(first=first)

    def _collect(self, row: List[int], n_prompt: int, seq, n: dict) -> List[int]:
        """The tokens a finished row emitted, from its line `row` of the `_tokens` array and its synced counts `n`."""
        self.cache.advance(seq, n["n_out"])  # the keys the device wrote: one per decode step the row took
        return row[:n["n_out"]]

    def _request(self, *args, **kw) -> Request:
        """The request object of one generate() call, from Request's own arguments: a subclass builds its own kind."""
        return Request(*args, **kw)

    def _admit_state(self, req: Request, q: int) -> dict:
        """What an admitted row writes besides _row_state, from the request's knowledge of its completion q: its prompt's adapter slot."""
        if self.lora is None:
            return {}
        slot = req.slots[q // self.family]
        return dict(lora_slot=slot if self.group == 1 else [slot] * self.group)

    def _settle(self, req: Request, q: int, n: dict) -> None:
        """A finished row's synced values `n` that the request keeps for its completion q: none here."""

    def _reset(self) -> None:
        """What the cleanup after an exception resets beyond `_idle`: nothing here."""

    # ---- the loop

    @torch.no_grad()
    def generate(self, prompts: Sequence[Sequence[int]], max_new_tokens: int, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                 generator: Optional[torch.Generator] = None, eos_token_id: Optional[int] = None,
                 adapters: Optional[Sequence[Optional[int]]] = None, repetition_penalty: float = 1.0,
                 presence_penalty: float = 0.0, frequency_penalty: float = 0.0, stop: Optional[Sequence[Sequence[int]]] = None,
                 stop_token_ids: Optional[Sequence[int]] = None, min_new_tokens: int = 0) -> List[List[int]]:
        """QuantLlamaForCausalLM.generate's contract -- up to `max_new_tokens` ids per prompt, the eos that ends a sequence included --
        served by this loop's rows: waiting prompts are admitted into idle rows, in order, whenever the pool's free blocks cover a
        prompt's whole budget (taken at once with PagedKVCache.reserve), prefilled eagerly in one packed step with their first token from
        ops.sample_tokens, and decoded by the captured step.  A prompt whose len + max_new_tokens - 1 exceeds max_len raises before
        anything runs.  The random draws: one torch.rand per prefill pass, one torch.rand(rows, u_stride) at the
        first decode step of the call and then per u_stride decode steps, so equally seeded generators give equal tokens whatever the
        loop served before.

        A loop built with family=N > 1 returns N completions per prompt (a list of N lists).  A prompt is admitted when a whole slot of N
        rows is idle and the pool covers the family: the prompt's budget once and, per further sibling, the blocks beyond the prompt's
        full ones.  It is prefilled once; its N first tokens are N draws from the one logits row (one torch.rand of admitted prompts * N
        per prefill pass), and the siblings that go on are made with PagedKVCache.fork and reserve.

        SpecDecodeLoop: the budget is len(prompt) + max_new_tokens - 1 + draft_len keys per sequence (reserved at once; the same sum must
        not exceed max_len).  The host writes an admitted row's history (the prompt and its first token) and first drafts (ngram_draft);
        everything after that happens on the device.  u is refilled whenever it is used up; a step uses draft_len + 1 variates per row,
        so sampled tokens differ from DecodeLoop's under the same seed.

        repetition_penalty, presence_penalty, frequency_penalty (1, 0, 0: none) need a loop built with penalties=True, whose step runs
        ops.penalize_logits between the forward and the sampler: every draw is made from logits penalised over the row's prompt and
        emitted tokens (include/qqq_amd_penalty.h) -- the first one from the prefill's logits penalised over the prompt, where every
        index is a prompt index and the repetition rule alone acts; a draft's logits row over the drafts in front of it too.

        A loop built with logprobs=k returns (tokens, records): `records` mirrors the nesting of `tokens` and holds per completion a
        TokenLogprobs of CPU tensors, one entry per emitted token, the eos included.  The first token's record comes from
        ops.topk_logprobs on the prefill's logits (Request.sample), the others from the step's ops.topk_logprobs_step; all of them are taken
        from the logits row the sampler drew from -- after the penalties, before temperature, top-k and top-p.  A finished row's
        records are read back with its tokens; the run itself gains no host sync.

        stop, stop_token_ids, min_new_tokens (None, None, 0: none; QuantLlamaForCausalLM.generate states their meaning) need a loop built
        with stops=True.  The call writes the stop table and the stop ids once; the step bans eos and the stop ids below the minimum
        (ops.ban_tokens) and retires a row whose completion ends in a stop id or a stop sequence (ops.stop_check, which is given the rows'
        eos too: a row the sampler retired on its eos keeps that token where a sequence ends in it), and a sync reads n_trim with the
        counts: the tokens -- and records -- a finished row drops from its end.  admit() does the same for the first token by the host
        path's own routines: Request.sample bans on the prefill's logits, and Request.receive ends a completion on its first token (a
        length-1 stop sequence that matches it leaves an empty completion whose row never starts).  The keys the device wrote are still
        counted by n_out.

        adapters (None: no prompt has one) needs a loop built with lora=bank: one slot of the bank or None per prompt.  The admission
        prefill carries the prompts' slots per token, an admitted row writes its slot into lora_slot and a finished one -1; the
        siblings of a family inherit their prompt's."""
        name = f"{self._name}.generate"
        if adapters is not None and self.lora is None:
            raise ValueError(f"{name}: adapters need a loop built with lora=bank")
        req = self._request(name, self.lm.lm_head.weight.shape[0], temperature, top_k, top_p, generator, eos_token_id, repetition_penalty,
                            presence_penalty, frequency_penalty, stop, stop_token_ids, min_new_tokens, self.family, self.logprobs,
                            lora=self.lora, adapters=adapters)
        if req.stopping and not self.stops:
            raise ValueError(f"{name}: stop, stop_token_ids and min_new_tokens={req.least} need a loop built with stops=True")
        if req.penalised and not self.penalties:
            raise ValueError(f"{name}: repetition_penalty={req.penalty[0]}, presence_penalty={req.penalty[1]} and "
                             f"frequency_penalty={req.penalty[2]} need a loop built with penalties=True")
        fam, max_new_tokens = self.family, int(max_new_tokens)
        prompts, outs = req.begin(prompts)  # outs, per sibling: prompt i's are i * fam ... i * fam + fam - 1
        if max_new_tokens < 1 or not prompts:
            return req.result()
        extra, new_words, parts = self._budget_words(max_new_tokens)
        keys = [len(p) + max_new_tokens - 1 + extra for p in prompts]
        for p, k in zip(prompts, keys):
            if k > self.max_len:
                raise ValueError(f"{name}: a prompt of {len(p)} tokens{new_words} need {k} keys, the loop was built for max_len={self.max_len}")
        if self.graph and self._graph is None:
            self._capture()
        self._start_call()
        cache, dev, bs = self.cache, self.device, self.cache.block_size
        tag = object()  # sequence ids no other user of the cache can hold
        sid = lambda i: (tag, i)  # noqa: E731
        waiting = deque(range(len(prompts)))
        owner: List[Optional[int]] = [None] * self.rows  # the sequence (prompt * fam + sibling) each row serves
        blocks = [req.family_blocks(len(p), k, bs) for p, k in zip(prompts, keys)]  # what a prompt's family takes
        budget = [0] * self.rows                         # an upper bound of the row's `remaining`, and so of the steps it still takes
        per_row = dict(remaining=max_new_tokens - 1, eos=req.eos, n_out=0, temperature=float(temperature), top_k=int(top_k), top_p=float(top_p))
        if self.penalties:
            per_row.update(zip(("repetition", "presence", "frequency"), req.penalty))
        if req.records is not None:
            per_row.update(n_rec=0)  # with n_out: the step's records are counted like its tokens
        synced_arrays = self._synced + (("n_trim",) if self.stops else ())
        if self.stops:  # the tables of the call, once; a row starts with its first token checked (by admit) and nothing to drop
            self.stop_ids.copy_(torch.tensor([s + [0] * (32 - len(s)) for s in req.stops] + [[0] * 32] * (32 - len(req.stops)), dtype=torch.int32))
            self.stop_len.copy_(torch.tensor([len(s) for s in req.stops] + [0] * (32 - len(req.stops)), dtype=torch.int32))
            self.ban_ids.copy_(torch.tensor(req.end_ids + [-1] * (32 - len(req.end_ids)), dtype=torch.int32))
            per_row.update(min_new=req.least, n_seen=1, n_trim=0, stop_hit=-1)

        def admit():
            new = []
            idle = [r for r in range(0, self.rows, fam) if all(o is None for o in owner[r:r + fam])]  # the first rows of idle slots
            pending = 0  # blocks the siblings of this round's prompts take once they are forked
            while waiting and idle:
                i = waiting[0]
                if blocks[i] > cache.free_blocks - pending:
                    break
                waiting.popleft()
                cache.add(sid(i * fam))
                cache.reserve(sid(i * fam), keys[i])
                pending += blocks[i] - -(-keys[i] // bs)
                owner[idle[0]] = i * fam
                new.append((idle.pop(0), i))
            if not new:
                if waiting and all(o is None for o in owner):
                    raise RuntimeError(f"{name}: the pool's {cache.free_blocks} free blocks cannot hold a prompt that needs "
                                       f"{blocks[waiting[0]]} ({parts})")
                return
            # the packed prefill of the admitted prompts (eager, the existing step) and their first tokens
            ids = torch.tensor([t for _, i in new for t in prompts[i]], dtype=torch.int64, device=dev)
            step = cache.step([sid(i * fam) for _, i in new], [len(prompts[i]) for _, i in new])
            logits = self.lm(ids, cache, req.with_adapters(step, [i for _, i in new], step.counts))
            born = [(r + j, i * fam + j) for r, i in new for j in range(fam)]  # (row, sequence) of every sibling
            first = req.sample(logits, [q for _, q in born], self.penalty_workspace if self.penalties else None)
            rows, state, ended = [], {}, []
            for (r, q), t in zip(born, first.tolist()):
                if req.receive(q, t, max_new_tokens):  # also on a stop sequence of length 1: an empty completion
                    if q % fam == 0:
                        ended.append((r, q))  # its siblings are forked from it first
                    continue
                prompt = prompts[q // fam]
                if q % fam:  # a sibling that goes on: the prompt's full blocks in common, the rest of its budget its own
                    cache.fork(sid(q - q % fam), sid(q))
                    owner[r] = q
                    cache.reserve(sid(q), keys[q // fam])
                rows.append(r)
                for array, value in dict(self._row_state(prompt, t, cache.blocks(sid(q))), **self._admit_state(req, q)).items():
                    state.setdefault(array, []).append(value)
                if fam > 1:
                    state.setdefault("shared", []).append(len(prompt) // bs * bs)
                budget[r] = max_new_tokens - 1
            for r, q in ended:
                cache.free(sid(q))
                owner[r] = None
            if not rows:
                return
            at = torch.tensor(rows, dtype=torch.int64, device=dev)
            for array, values in state.items():
                dst = getattr(self, array)
                dst[at] = torch.tensor(values, dtype=dst.dtype).to(dev)
            for array, value in per_row.items():  # the same for every row of the call, and for each of a row's logits rows
                getattr(self, array).view(self.rows, -1)[at] = value

        try:
            while True:
                admit()
                active = [r for r in range(self.rows) if owner[r] is not None]
                if not active:
                    if waiting:
                        continue
                    break
                self._run(min(self.sync_every, max(budget[r] for r in active)), generator)
                synced = dict(zip(synced_arrays, torch.stack([getattr(self, a) for a in synced_arrays]).tolist()))  # the sync: one transfer
                remaining = synced["remaining"]
                done = [r for r in active if remaining[r] == 0]
                for r in active:
                    budget[r] = remaining[r]
                if done:
                    at_done = torch.tensor(done, dtype=torch.int64, device=dev)
                    toks = getattr(self, self._tokens)[at_done].tolist()
                    if req.records is not None:  # read back with the tokens: record j of a row belongs to out[r, j]
                        lp = [a[at_done].cpu() for a in (self.lp, self.lp_rank, self.lp_top_ids, self.lp_top)]
                        for j, r in enumerate(done):
                            req.records.tail[owner[r]] = tuple(p[j, :synced["n_out"][r]] for p in lp)
                    for r, row in zip(done, toks):
                        i = owner[r]
                        outs[i].extend(self._collect(row, len(prompts[i // fam]), sid(i), {a: v[r] for a, v in synced.items()}))
                        if self.stops:  # what ops.stop_check found behind the completion's end
                            req.cut(i, synced["n_trim"][r])
                        self._settle(req, i, {a: v[r] for a, v in synced.items()})
                        cache.free(sid(i))
                        owner[r] = None
                    if fam > 1:
                        self.shared[at_done] = 0
                    if self.lora is not None:
                        self.lora_slot[at_done] = -1
        except BaseException:
            # leave the loop idle and the caller's pool as it was found
            for i in owner:
                if i is not None:
                    cache.free(sid(i))
            for array, value in self._idle + ((("shared", 0),) if fam > 1 else ()) + ((("lora_slot", -1),) if self.lora is not None else ()):
                getattr(self, array).fill_(value)
            if req.records is not None:
                self.n_rec.copy_(self.n_out)  # no row owes a record
            if self.stops:
                self.n_seen.copy_(self.n_out + 1)  # ... or a check
                self.n_trim.zero_()
            self._reset()
            raise
        return req.result()


class GuidedDecodeLoop(DecodeLoop):
    """DecodeLoop whose rows follow token automata (qqq_amd/guided.py) held in device memory: the step runs ops.fsm_mask between the ban and
    the sampler and ops.fsm_advance behind the stop check, inside the captured graph, so a guided completion costs no host sync per token.

    fsm_states, fsm_edges   the capacities of the loop's CSR buffers: fsm_offsets int32 [fsm_states + 1], fsm_tokens / fsm_next int32
                [fsm_edges], fsm_accept int32 [fsm_states].  Every generate_guided() copies its (merged) automaton into them, as the stop
                table is copied, and the ops are launched with the capacities: one capture serves every call.  An automaton that exceeds
                them raises before anything runs.
    The loop owns fsm_state (int32 [rows]: a row's state; -1 when idle or unconstrained, -2 once a token outside the automaton was drawn)
    and n_fsm (int32 [rows]: the count of emitted tokens up to which fsm_state has been advanced).  Admission masks the prefill's logits
    and steps the first token on the host (GuidedRequest) and writes fsm_state and n_fsm = 0; a first token that already reaches a terminal
    state ends the completion there and the row never starts.  fsm_state is read back with the counts at every sync.  penalties, family,
    logprobs and stops are DecodeLoop's.  generate() serves unconstrained calls; generate_guided() takes the automata."""

    _name = "GuidedDecodeLoop"
    _synced = DecodeLoop._synced + ("fsm_state",)
    _idle = DecodeLoop._idle + (("fsm_state", -1),)

    def __init__(self, lm, cache: PagedKVCache, rows: int, max_len: int, fsm_states: int = 1024, fsm_edges: int = 65536, sync_every: int = 8,
                 u_stride: int = 64, graph: bool = True, penalties: bool = False, family: int = 1, logprobs: Optional[int] = None,
                 stops: bool = False):
        fsm_states, fsm_edges = int(fsm_states), int(fsm_edges)
        if fsm_states < 1 or fsm_edges < 1:
            raise ValueError(f"GuidedDecodeLoop: fsm_states={fsm_states} and fsm_edges={fsm_edges} must be at least 1")
        super().__init__(lm, cache, rows, max_len, sync_every=sync_every, u_stride=u_stride, graph=graph, penalties=penalties, family=family,
                         logprobs=logprobs, stops=stops)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.fsm_states, self.fsm_edges = fsm_states, fsm_edges
        self.fsm_state = torch.full((self.rows,), -1, **i32)
        self.n_fsm = torch.zeros(self.rows, **i32)
        self.fsm_offsets = torch.zeros(fsm_states + 1, **i32)
        self.fsm_tokens = torch.zeros(fsm_edges, **i32)
        self.fsm_next = torch.zeros(fsm_edges, **i32)
        self.fsm_accept = torch.zeros(fsm_states, **i32)
        self._tables = (self.fsm_offsets, self.fsm_tokens, self.fsm_next, self.fsm_accept)
        self._given = self._guided = None

    def _before_sample(self, logits: torch.Tensor) -> None:
        ops.fsm_mask(logits, self.fsm_state, self._tables, eos=self.eos, remaining=self.remaining)

    def _after_sample(self, logits: torch.Tensor) -> None:
        ops.fsm_advance(self.out, self.n_out, self.n_fsm, self.fsm_state, self._tables, self.ids, self.pos, self.slots, self.remaining,
                        eos=self.eos)

    def _request(self, *args, **kw) -> Request:
        self._guided = GuidedRequest(self._given, *args, **kw)
        return self._guided

    def _start_call(self) -> None:
        """the call's automaton into the loop's buffers, once: the states beyond it have no edges and nothing leads to them"""
        super()._start_call()
        fsm = self._guided.fsm  # (generate_guided has held it against the capacities)
        pad = lambda a, size, fill: torch.cat([torch.from_numpy(a), torch.full((size - a.shape[0],), fill, dtype=torch.int32)])  # noqa: E731
        self.fsm_offsets.copy_(pad(fsm.offsets, self.fsm_states + 1, fsm.n_edges))
        self.fsm_tokens.copy_(pad(fsm.tokens, self.fsm_edges, 0))
        self.fsm_next.copy_(pad(fsm.next, self.fsm_edges, 0))
        self.fsm_accept.copy_(pad(fsm.accept, self.fsm_states, 0))

    def _too_large(self, fsm) -> str:
        return (f"{self._name}.generate_guided: an automaton of {fsm.n_states} states and {fsm.n_edges} edges exceeds the loop's capacities "
                f"fsm_states={self.fsm_states} and fsm_edges={self.fsm_edges}")

    def _admit_state(self, req: Request, q: int) -> dict:
        return dict(fsm_state=req.state[q], n_fsm=0)

    def _settle(self, req: Request, q: int, n: dict) -> None:
        req.state[q] = n["fsm_state"]

    def _reset(self) -> None:
        self.n_fsm.copy_(self.n_out)  # no row owes an advance

    @torch.no_grad()
    def generate_guided(self, prompts: Sequence[Sequence[int]], fsm, max_new_tokens: int, *args, **kw):
        """generate() with every completion held to `fsm`: one TokenFSM for all prompts, or a sequence with one entry per prompt (None:
        unconstrained); the further arguments are generate()'s.  The merged automaton must fit the loop's capacities, or the call raises
        ValueError before anything runs.  A completion that left its automaton (every allowed logit -inf or NaN) makes the call raise
        RuntimeError once the pool is left as it was found and the loop idle."""
        prompts = [list(p) for p in prompts]
        merged, _ = merge_automata(f"{self._name}.generate_guided", fsm, len(prompts))
        if merged.n_states > self.fsm_states or merged.n_edges > self.fsm_edges:
            raise ValueError(self._too_large(merged))
        self._given = fsm
        try:
            result = self.generate(prompts, max_new_tokens, *args, **kw)
        finally:
            self._given = None
        self._guided.check()
        return result


def ngram_draft(history: Sequence[int], draft_len: int, ngram_max: int = 3) -> List[int]:
    """The `draft_len` tokens guessed to follow `history` by prompt lookup, the rule of include/qqq_amd_spec.h: for n = ngram_max down to 1
    (only while n < len(history)) the latest earlier occurrence of the last n tokens; the first n that has one wins and the draft is what
    followed it, copied with overlap (a match that runs into the end of the history continues its period).  With no match at all the
    last token repeats.  Deterministic; ops.spec_advance computes the same tokens on the device."""
    h = [int(t) for t in history]
    draft_len, ngram_max, n_h = int(draft_len), int(ngram_max), len(h)
    if not h or draft_len < 1 or ngram_max < 1:
        raise ValueError("ngram_draft: history must hold a token, draft_len and ngram_max must be at least 1")
    src = None
    for n in range(min(ngram_max, n_h - 1), 0, -1):
        tail = h[n_h - n:]
        src = next((i + n for i in range(n_h - n - 1, -1, -1) if h[i:i + n] == tail), None)
        if src is not None:
            break
    if src is None:
        return [h[-1]] * draft_len
    out: List[int] = []
    for j in range(draft_len):
        out.append(h[src + j] if src + j < n_h else out[src + j - n_h])
    return out


def _takes_verify(attn, group: int) -> bool:
    """fuse_verify() is set on `attn` and its kernel takes a chunk of `group` tokens per row"""
    return getattr(attn, "_verify", False) and 2 <= group <= 16 and (attn.num_heads // attn.num_key_value_heads) * group <= 64


class SpecDecodeLoop(DecodeLoop):
    """DecodeLoop with speculation: every row feeds its last token and `draft_len` drafted tokens through one forward pass (a chunk of
    G = draft_len + 1 tokens per row through the paged prefill attention kernel, every token's logits), and ops.spec_advance draws a token
    from each logits row, emits the draws behind a rightly guessed prefix -- 1 ... G tokens per row and step -- drafts the next chunk by
    n-gram lookup in the row's history (ngram_draft) and advances or retires the row, all on the device.  The step is one captured graph
    as in DecodeLoop.  Every emitted token is a plain sampler draw from logits computed on the true prefix: the output distribution is
    DecodeLoop's at any temperature, top_k and top_p.  The tokens under a seed are not: a step uses G variates per row.  Greedy tokens
    are DecodeLoop's up to near-ties of the logits (the head GEMM runs at another row count).

    The model must have fuse_prefill() or fuse_verify() set: the per-sequence SDPA path reads lengths on the host.  With fuse_verify() the
    step's chunk takes the verify attention kernel, whose rows are bit for bit the decode steps'; admission prefill stays as it is.  A
    sequence needs
    len(prompt) + max_new_tokens - 1 + draft_len keys of the pool and of max_len: the drafts behind its last token are written too.
    ngram_max   the longest n-gram the drafter looks up (1 ... 4);  u_stride  default sync_every * G, a multiple of G
    lora        as in DecodeLoop, with lora_slot [rows, draft_len + 1]: the row's slot repeated over its chunk
    penalties   as in DecodeLoop, with `seen` being `hist` itself: logits row j of a row is penalised over its history and the drafts
                1 ... j in front of it, so an emitted token is still a plain sampler draw from (penalised) logits of the true prefix
    After a generate(): `accepted` drafts were accepted in `row_steps` steps of single rows, over `steps` steps of the loop; a row-step
    emits 1 + its accepted drafts tokens."""

    _name = "SpecDecodeLoop"
    _tokens = "hist"
    _synced = ("n_out", "remaining", "n_acc")
    _idle = DecodeLoop._idle + (("start", -1),)

    def __init__(self, lm, cache: PagedKVCache, rows: int, max_len: int, draft_len: int = 4, ngram_max: int = 3, sync_every: int = 8,
                 u_stride: Optional[int] = None, graph: bool = True, penalties: bool = False, family: int = 1, lora=None,
                 stops: bool = False):
        rows, max_len, sync_every, draft_len, ngram_max = int(rows), int(max_len), int(sync_every), int(draft_len), int(ngram_max)
        if int(family) != 1:
            raise ValueError(f"SpecDecodeLoop: family={family} is not supported (a chunk of draft_len + 1 tokens per row has no "
                             f"shared-prefix kernel); DecodeLoop takes families")
        if draft_len < 1 or draft_len > 15 or ngram_max < 1 or ngram_max > 4:
            raise ValueError(f"SpecDecodeLoop: draft_len={draft_len} must be in [1, 15] and ngram_max={ngram_max} in [1, 4]")
        group = draft_len + 1
        if u_stride is None:
            u_stride = max(sync_every, 1) * group
        u_stride = int(u_stride)
        short = u_stride < sync_every * group and (f"u_stride={u_stride} must cover the sync_every={sync_every} steps between two refills, "
                                                   f"draft_len + 1 = {group} variates each")
        dev = _check_loop("SpecDecodeLoop", lm, cache, rows, max_len, sync_every, graph, short)
        if rows * group > 65535:
            raise ValueError(f"SpecDecodeLoop: rows={rows} times draft_len + 1 = {group} exceeds the sampler's 65535 logits rows")
        if max_len <= draft_len:
            raise ValueError(f"SpecDecodeLoop: max_len={max_len} must exceed draft_len={draft_len}")
        if not all(getattr(layer.self_attn, "_prefill", False) or _takes_verify(layer.self_attn, group) for layer in lm.model.layers):
            raise RuntimeError("SpecDecodeLoop: the model needs fuse_prefill() or fuse_verify(): a step is a chunk of draft_len + 1 tokens per "
                               "row, and only the paged prefill and the verify attention kernels serve chunks without reading lengths on the "
                               "host (fuse_verify() alone takes chunks of (h / kvh) * (draft_len + 1) <= 64 query rows)")
        self.draft_len, self.ngram_max, self.group = draft_len, ngram_max, group
        self.accepted = self.row_steps = self.steps = 0
        self._allocate(lm, cache, rows, max_len, sync_every, u_stride, graph, dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.start = torch.full((rows,), -1, dtype=torch.int64, device=dev)
        self.hist = torch.zeros((rows, max_len), **i32)
        self.hist_len = torch.zeros(rows, **i32)
        self.n_acc = torch.zeros(rows, **i32)
        if penalties:  # the history the drafter reads is what the rows have seen; the op's write into it is the identity
            self._allocate_penalties(self.hist)
        if stops:  # the completion is what follows the prompt in hist: stop_base is the prompt's length, written on admission
            self._allocate_stops(0)
        # the one step of every pass: a chunk of G tokens per row whose device tensors ARE the state arrays
        self.step = PagedStep(seq_ids=[None] * rows, counts=[group] * rows, starts=[0] * rows, max_len=max_len, decode=False,
                              pos=self.pos.view(-1), slots=self.slots.view(-1), block_table=self.block_table, last_pos=self.start,
                              cu_tokens=torch.arange(rows + 1, **i32) * group, start_pos=self.start)
        if lora is not None:  # lora_slot [rows, draft_len + 1]: the row's slot on every token of its chunk
            self._allocate_lora(lora)

    def _decode_step(self) -> None:
        logits = self.lm(self.ids.view(-1), self.cache, self.step, all_rows=True)
        if self.penalties:
            self._penalize(logits)
        if self.stops:  # logits row j of a row is the one its completion's token n_out + 1 + j is drawn from
            self._ban(logits)
        ops.spec_advance(logits, self.temperature, self.top_k, self.top_p, self.u, self.tick, self.ids, self.pos, self.slots, self.start,
                         self.block_table, self.remaining, self.eos, self.hist, self.hist_len, self.n_out, self.n_acc,
                         self.cache.block_size, self.ngram_max)
        if self.stops:  # every length the step added, in order: the tokens behind a match are dropped with it
            self._stop_check()

    def _stop_check(self) -> None:
        ops.stop_check(self.hist, self.stop_base, None, self.n_out, self.stop_ids, self.stop_len, self.min_new, self.n_seen, self.n_trim,
                       self.stop_hit, self.ids, self.pos, self.slots, self.remaining, start=self.start, end_ids=self.ban_ids, eos=self.eos)

    def _run(self, steps: int, generator) -> None:
        super()._run(steps, generator)
        self.steps += steps

    def _start_call(self) -> None:
        super()._start_call()
        self.accepted = self.row_steps = self.steps = 0

    def _budget_words(self, new: int):
        return self.draft_len, f", {new} new ones and {self.draft_len} drafts", "prompt, budget and drafts"  # the drafts are written too

    def _row_state(self, prompt: List[int], first: int, blocks: List[int]) -> dict:
        p, bs, h = len(prompt), self.cache.block_size, prompt + [first]
        chunk = range(p, p + self.group)
        return dict(super()._row_state(prompt, first, blocks), ids=[first] + ngram_draft(h, self.draft_len, self.ngram_max), pos=list(chunk),
                    slots=[blocks[q // bs] * bs + q % bs for q in chunk], start=p, n_acc=0, hist=h + [0] * (self.hist.shape[1] - len(h)),
                    hist_len=len(h))

    def _penalty_state(self, prompt: List[int]) -> dict:
        return dict(n_prompt=len(prompt))  # `seen` is hist

    def _stop_state(self, prompt: List[int], first: int) -> dict:
        return dict(stop_base=len(prompt))  # the first token is hist[len(prompt)]

    def _collect(self, row: List[int], n_prompt: int, seq, n: dict) -> List[int]:
        self.accepted += n["n_acc"]
        self.row_steps += n["n_out"] - n["n_acc"]  # a row-step emits one token more than it accepts drafts
        first = n_prompt + 1  # the prompt and the prefill's token
        return row[first:first + n["n_out"]]


__all__ = ["DecodeLoop", "GuidedDecodeLoop", "SpecDecodeLoop", "ngram_draft"]
