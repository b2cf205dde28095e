"""The device-resident decode loop: a fixed number of rows whose per-step metadata lives in device memory and is advanced there by
ops.sample_advance, so that one decode step -- model forward + sample_advance -- reads nothing on the host and is ONE captured graph,
replayed `sync_every` times between host syncs while rows finish and join without re-capture.

    DecodeLoop   the rows' state arrays (include/qqq_amd_step.h), the one PagedStep built over them, the captured step, and generate()

QuantLlamaForCausalLM.generate (qqq_amd/model.py) builds its batch anew on the host for every token: a PagedKVCache.step, an eager launch
of every kernel, a tolist() before the next step.  Here the host only admits prompts (an eager packed prefill, the first token from
ops.sample_tokens), writes the admitted rows' state with indexed copies, replays, and reads (n_out, remaining) back once per `sync_every`
steps.  A row that is idle (pos -1, slot -1, remaining 0) rides along in every step and is inert: see include/qqq_amd_step.h.
"""
from __future__ import annotations

from collections import deque
from typing import List, Optional, Sequence

import torch

from . import ops
from .paged import PagedKVCache, PagedStep


class DecodeLoop:
    """`rows` decode rows over `cache` for sequences of at most `max_len` keys (prompt and generated tokens but the last).

    lm          a QuantLlamaForCausalLM on the GPU;  cache  a PagedKVCache of its shape (it may hold other sequences)
    rows        the batch of every decode step, idle rows included; fixed, as is max_len: the decode kernel's split plan is a function of
                (rows, kv heads, max_len), so a captured step holds for exactly these two
    sync_every  decode steps between two host syncs;  u_stride  uniform variates per row and refill (>= sync_every)
    graph       True: the step is captured once into a torch.cuda.CUDAGraph (on a side stream; single-stream, straight-line) and replayed;
                False: the same calls run eagerly.  Both give the same tokens.
    `captures` counts the captures: 1 for the life of the loop with graph=True.  The graph holds addresses: a model that is changed after
    the first generate() (fuse_*(), load_state_dict, .to()) needs a new loop."""

    def __init__(self, lm, cache: PagedKVCache, rows: int, max_len: int, sync_every: int = 8, u_stride: int = 64, graph: bool = True):
        if not isinstance(cache, PagedKVCache):
            raise TypeError("DecodeLoop: cache must be a PagedKVCache")
        rows, max_len, sync_every, u_stride = int(rows), int(max_len), int(sync_every), int(u_stride)
        if rows < 1 or rows > 65535 or max_len < 1 or sync_every < 1:
            raise ValueError(f"DecodeLoop: rows={rows}, max_len={max_len} and sync_every={sync_every} must be at least 1 (rows <= 65535)")
        if u_stride < sync_every:
            raise ValueError(f"DecodeLoop: u_stride={u_stride} must cover the sync_every={sync_every} steps between two refills")
        if max_len > cache.capacity:
            raise ValueError(f"DecodeLoop: max_len={max_len} exceeds what the pool could hold ({cache.capacity} keys)")
        dev = lm.lm_head.weight.device
        if cache.k[0].device != dev:
            raise RuntimeError("DecodeLoop: the model and the cache must be on the same device")
        if graph and dev.type != "cuda":
            raise RuntimeError("DecodeLoop: graph=True needs the model on the GPU (and the ops of a step have no CPU path)")
        self.lm, self.cache, self.rows, self.max_len, self.sync_every, self.u_stride = lm, cache, rows, max_len, sync_every, u_stride
        self.graph, self.device, self.captures = bool(graph), dev, 0
        bs = cache.block_size
        i32 = dict(dtype=torch.int32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        self.ids = torch.zeros(rows, **i64)
        self.pos = torch.full((rows,), -1, **i64)
        self.slots = torch.full((rows,), -1, **i64)
        self.block_table = torch.zeros((rows, -(-max_len // bs)), **i32)
        self.remaining = torch.zeros(rows, **i32)
        self.eos = torch.full((rows,), -1, **i32)
        self.out = torch.zeros((rows, max_len), **i64)
        self.n_out = torch.zeros(rows, **i32)
        self.tick = torch.zeros(rows, **i32)
        self.u = torch.zeros((rows, u_stride), dtype=torch.float32, device=dev)
        self.temperature = torch.zeros(rows, dtype=torch.float32, device=dev)
        self.top_k = torch.zeros(rows, **i32)
        self.top_p = torch.ones(rows, dtype=torch.float32, device=dev)
        # the one step of every decode pass: its device tensors ARE the state arrays (a row's position is its last position)
        self.step = PagedStep(seq_ids=[None] * rows, counts=[1] * rows, starts=[0] * rows, max_len=max_len, decode=True, pos=self.pos,
                              slots=self.slots, block_table=self.block_table, last_pos=self.pos,
                              cu_tokens=torch.arange(rows + 1, **i32), start_pos=self.pos)
        self._graph = None
        self._used = u_stride  # variates of u consumed since its last refill: none are left

    # ---- one decode step

    def _decode_step(self) -> None:
        logits = self.lm(self.ids, self.cache, self.step)
        ops.sample_advance(logits, self.temperature, self.top_k, self.top_p, self.u, self.tick, self.ids, self.pos, self.slots,
                           self.block_table, self.remaining, self.eos, self.out, self.n_out, self.cache.block_size)

    def _capture(self) -> None:
        """Warm up and capture the step with every row idle (nothing but `tick` changes), on a side stream."""
        if bool((self.remaining != 0).any()):
            raise RuntimeError("DecodeLoop: the step is captured with every row idle")
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
        if self._used + steps > self.u_stride:  # tick is about to wrap: new variates, and the rows start over at the first
            self.u.copy_(torch.rand((self.rows, self.u_stride), generator=generator, device=self.device))
            self.tick.zero_()
            self._used = 0
        self._used += steps
        for _ in range(steps):
            if self._graph is not None:
                self._graph.replay()
            else:
                self._decode_step()

    # ---- the loop

    @torch.no_grad()
    def generate(self, prompts: Sequence[Sequence[int]], max_new_tokens: int, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                 generator: Optional[torch.Generator] = None, eos_token_id: Optional[int] = None) -> List[List[int]]:
        """QuantLlamaForCausalLM.generate's contract -- up to `max_new_tokens` ids per prompt, the eos that ends a sequence included --
        served by this loop's rows: waiting prompts are admitted into idle rows, in order, whenever the pool's free blocks cover a
        prompt's whole budget (taken at once with PagedKVCache.reserve), prefilled eagerly in one packed step with their first token from
        ops.sample_tokens, and decoded by the captured step.  A prompt whose len + max_new_tokens - 1 exceeds max_len raises before
        anything runs.  The random draws: one torch.rand per prefill pass, one torch.rand(rows, u_stride) at the
        first decode step of the call and then per u_stride decode steps, so equally seeded generators give equal tokens whatever the
        loop served before."""
        prompts = [list(p) for p in prompts]
        if any(not p for p in prompts):
            raise ValueError("DecodeLoop.generate: every prompt needs at least one token")
        outs: List[List[int]] = [[] for _ in prompts]
        max_new_tokens = int(max_new_tokens)
        if max_new_tokens < 1 or not prompts:
            return outs
        for p in prompts:
            if len(p) + max_new_tokens - 1 > self.max_len:
                raise ValueError(f"DecodeLoop.generate: a prompt of {len(p)} tokens and {max_new_tokens} new ones need "
                                 f"{len(p) + max_new_tokens - 1} keys, the loop was built for max_len={self.max_len}")
        if self.graph and self._graph is None:
            self._capture()
        self._used = self.u_stride  # this call draws with its own generator alone: nothing an earlier call left in u is used
        cache, dev, bs = self.cache, self.device, self.cache.block_size
        eos = -1 if eos_token_id is None else int(eos_token_id)
        tag = object()  # sequence ids no other user of the cache can hold
        sid = lambda i: (tag, i)  # noqa: E731
        waiting = deque(range(len(prompts)))
        owner: List[Optional[int]] = [None] * self.rows  # the prompt each row serves
        budget = [0] * self.rows                         # an upper bound of the row's `remaining`

        def admit():
            new = []
            idle = [r for r in range(self.rows) if owner[r] is None]
            while waiting and idle:
                i = waiting[0]
                keys = len(prompts[i]) + max_new_tokens - 1
                if -(-keys // bs) > cache.free_blocks:
                    break
                waiting.popleft()
                cache.add(sid(i))
                cache.reserve(sid(i), keys)
                owner[idle[0]] = i
                new.append((idle.pop(0), i))
            if not new:
                if waiting and all(o is None for o in owner):
                    need = -(-(len(prompts[waiting[0]]) + max_new_tokens - 1) // bs)
                    raise RuntimeError(f"DecodeLoop.generate: the pool's {cache.free_blocks} free blocks cannot hold a prompt that needs "
                                       f"{need} (prompt and budget)")
                return
            # the packed prefill of the admitted prompts (eager, the existing step) and their first tokens
            seqs = [sid(i) for _, i in new]
            ids = torch.tensor([t for _, i in new for t in prompts[i]], dtype=torch.int64, device=dev)
            logits = self.lm(ids, cache, cache.step(seqs, [len(prompts[i]) for _, i in new]))
            u = torch.rand(len(new), generator=generator, device=dev)
            first = ops.sample_tokens(logits, temperature, top_k, top_p, u).tolist()
            rows, tok, pos, slots, rem, tables = [], [], [], [], [], []
            for (r, i), t in zip(new, first):
                outs[i].append(t)
                if max_new_tokens == 1 or t == eos:
                    cache.free(sid(i))
                    owner[r] = None
                    continue
                blocks, p = cache.blocks(sid(i)), len(prompts[i])
                rows.append(r)
                tok.append(t)
                pos.append(p)
                slots.append(blocks[p // bs] * bs + p % bs)
                rem.append(max_new_tokens - 1)
                tables.append(blocks + [0] * (self.block_table.shape[1] - len(blocks)))
                budget[r] = max_new_tokens - 1
            if not rows:
                return
            at = torch.tensor(rows, dtype=torch.int64, device=dev)
            n = len(rows)
            for dst, src, dtype in ((self.ids, tok, torch.int64), (self.pos, pos, torch.int64), (self.slots, slots, torch.int64),
                                    (self.remaining, rem, torch.int32), (self.eos, [eos] * n, torch.int32),
                                    (self.n_out, [0] * n, torch.int32), (self.block_table, tables, torch.int32),
                                    (self.temperature, [float(temperature)] * n, torch.float32), (self.top_k, [int(top_k)] * n, torch.int32),
                                    (self.top_p, [float(top_p)] * n, torch.float32)):
                dst[at] = torch.tensor(src, dtype=dtype).to(dev)

        try:
            while True:
                admit()
                active = [r for r in range(self.rows) if owner[r] is not None]
                if not active:
                    if waiting:
                        continue
                    break
                steps = min(self.sync_every, max(budget[r] for r in active))
                self._run(steps, generator)
                n_out, remaining = torch.stack((self.n_out, self.remaining)).tolist()  # the sync: one transfer
                done = [r for r in active if remaining[r] == 0]
                for r in active:
                    budget[r] = remaining[r]
                if done:
                    toks = self.out[torch.tensor(done, dtype=torch.int64, device=dev)].tolist()
                    for r, row in zip(done, toks):
                        i = owner[r]
                        outs[i].extend(row[:n_out[r]])
                        cache.advance(sid(i), n_out[r])  # the keys the device wrote: one per decode step the row took
                        cache.free(sid(i))
                        owner[r] = None
        except BaseException:
            # leave the loop idle and the caller's pool as it was found
            for r, i in enumerate(owner):
                if i is not None:
                    cache.free(sid(i))
            self.remaining.zero_()
            self.pos.fill_(-1)
            self.slots.fill_(-1)
            self.ids.zero_()
            raise
        return outs


__all__ = ["DecodeLoop"]
