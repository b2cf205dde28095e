"""The whole model around the quantised decoder layers: the reference's QuantizedLlamaModel / QuantizedLlamaForCausalLM and their Qwen2
twins (QQQ/gptq/models/llama.py, qwen2.py), and the generation loop of its examples/test_model.py over the paged KV cache.

    QuantLlamaModel        embed_tokens (fp16 nn.Embedding) -> layers (QuantLlamaDecoderLayer, chained through forward_chained: the add
                           that ends a layer is formed by the next layer's norm launch) -> norm (QuantRMSNorm): the normed fp16 rows
    QuantLlamaForCausalLM  model + lm_head (fp16 nn.Linear, not quantised, as in the reference): logits; generate(); score(),
                           loglikelihood() and perplexity() (qqq_amd/score.py), the reference's examples/eval_model.py

Parameter and buffer names are the reference's (model.embed_tokens.weight, model.layers.N. ..., model.norm.weight, lm_head.weight), so a
state-dict saved by it loads with load_state_dict(strict=True).

generate() serves prompts of different lengths in one batch over a PagedKVCache: the prompts are prefilled as one packed step, every later
step feeds each running sequence's last token, tokens come from ops.sample_tokens and stay on the device for the next embedding lookup, a
sequence that ends frees its blocks at once, and prompts the pool could not hold yet are admitted as blocks come free.
"""
from __future__ import annotations

from collections import deque
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, serve
from .attention import KVCache, QuantLlamaDecoderLayer
from .blocks import QuantRMSNorm
from .paged import PagedKVCache, PagedStep
from .request import GuidedRequest, Request, TokenLogprobs, stop_arguments, stop_match  # noqa: F401  (the last three: re-exported)


class QuantLlamaModel(nn.Module):
    """Quantized{Llama,Qwen2}Model: embedding, decoder layers, final norm.

    forward(input_ids, cache, step_or_start, all_rows=False) -> the normed fp16 hidden rows.
      PagedKVCache + PagedStep: input_ids int64 [m], packed as the step says -> [b, hidden], the last token of each sequence (rows
                                cu_tokens[1:] - 1, selected on the device); all_rows=True -> [m, hidden]
      KVCache + start position: input_ids int64 [b, s] -> [b, hidden]; all_rows=True -> [b, s, hidden]"""

    def __init__(self, vocab_size: int, num_layers: int, hidden: int, num_heads: int, num_kv_heads: int, intermediate: int, group_size: int,
                 rms_norm_eps: float = 1e-6, padding_idx: Optional[int] = None, layers: Optional[Sequence[nn.Module]] = None, **layer_kw):
        super().__init__()
        self.vocab_size, self.hidden_size = vocab_size, hidden
        self.embed_tokens = nn.Embedding(vocab_size, hidden, padding_idx, dtype=torch.float16)
        self.embed_tokens.weight.requires_grad_(False)
        if layers is None:
            layers = [QuantLlamaDecoderLayer(hidden, num_heads, num_kv_heads, intermediate, group_size, rms_norm_eps=rms_norm_eps,
                                             layer_idx=i, **layer_kw) for i in range(num_layers)]
        self.layers = nn.ModuleList(layers)
        self.norm = QuantRMSNorm(hidden, eps=rms_norm_eps)

    @classmethod
    def from_config(cls, config, group_size: int):
        """The model of a transformers LlamaConfig or Qwen2Config (duck-typed, as QuantLlamaDecoderLayer.from_config, whose refusals
        propagate)."""
        layers = [QuantLlamaDecoderLayer.from_config(config, group_size, layer_idx=i) for i in range(config.num_hidden_layers)]
        heads = config.num_attention_heads
        return cls(config.vocab_size, config.num_hidden_layers, config.hidden_size, heads, getattr(config, "num_key_value_heads", None) or heads,
                   config.intermediate_size, group_size, rms_norm_eps=config.rms_norm_eps, padding_idx=getattr(config, "pad_token_id", None),
                   layers=layers)

    def _each_layer(self, name: str):
        for layer in self.layers:
            getattr(layer, name)()
        return self

    def fuse_decode(self):
        """fuse_decode() on every layer.  Returns self."""
        return self._each_layer("fuse_decode")

    def unfuse_decode(self):
        return self._each_layer("unfuse_decode")

    def fuse_prefill(self):
        """fuse_prefill() on every layer.  Returns self."""
        return self._each_layer("fuse_prefill")

    def unfuse_prefill(self):
        return self._each_layer("unfuse_prefill")

    def fuse_verify(self):
        """fuse_verify() on every layer.  Returns self."""
        return self._each_layer("fuse_verify")

    def unfuse_verify(self):
        return self._each_layer("unfuse_verify")

    def fuse_shared(self):
        """fuse_shared() on every layer.  Returns self."""
        return self._each_layer("fuse_shared")

    def unfuse_shared(self):
        return self._each_layer("unfuse_shared")

    @property
    def shared_fused(self) -> bool:
        return all(layer.shared_fused for layer in self.layers)

    def fuse_qkv(self):
        """self_attn.fuse_qkv() on every layer (a second copy of the q / k / v weights).  Returns self."""
        for layer in self.layers:
            layer.self_attn.fuse_qkv()
        return self

    def unfuse_qkv(self):
        for layer in self.layers:
            layer.self_attn.unfuse_qkv()
        return self

    def forward(self, input_ids: torch.Tensor, cache, step_or_start, all_rows: bool = False) -> torch.Tensor:
        paged = isinstance(cache, PagedKVCache)
        if paged:
            if not isinstance(step_or_start, PagedStep):
                raise RuntimeError("QuantLlamaModel: a PagedKVCache takes the PagedStep of cache.step(seq_ids, counts)")
            if input_ids.dim() != 1 or input_ids.shape[0] != sum(step_or_start.counts):
                raise RuntimeError(f"QuantLlamaModel: input_ids must be [m] with the step's m = {sum(step_or_start.counts)} tokens packed in order")
        elif input_ids.dim() != 2 or input_ids.shape[0] != cache.batch:
            raise RuntimeError(f"QuantLlamaModel: input_ids must be [batch, s] with batch = {cache.batch} (the cache's)")
        delta, residual = self.embed_tokens(input_ids).reshape(-1, self.hidden_size), None
        for layer in self.layers:
            delta, residual = layer.forward_chained(delta, residual, cache, step_or_start)
        if not all_rows:  # the last token of every sequence, before the (row-wise) final norm
            if paged and not step_or_start.decode:
                rows = step_or_start.cu_tokens[1:].long() - 1
                delta = delta.index_select(0, rows)
                residual = residual.index_select(0, rows) if residual is not None else None
            elif not paged and input_ids.shape[1] > 1:
                b, s = input_ids.shape
                delta = delta.reshape(b, s, -1)[:, -1].contiguous()
                residual = residual.reshape(b, s, -1)[:, -1].contiguous() if residual is not None else None
        w = self.norm.weight if self.norm.weight.dtype == torch.float16 else self.norm.weight.half()
        y = ops.rmsnorm_quant(delta, w, self.norm.variance_epsilon, residual=residual, return_y=True)[2]
        if not paged and all_rows:
            return y.reshape(input_ids.shape + (self.hidden_size,))
        return y


class QuantLlamaForCausalLM(nn.Module):
    """Quantized{Llama,Qwen2}ForCausalLM: QuantLlamaModel and an fp16 lm_head.  forward(...) takes QuantLlamaModel.forward's arguments and
    returns the fp16 logits of the rows it returns."""

    def __init__(self, model: QuantLlamaModel, tie_word_embeddings: bool = False):
        super().__init__()
        self.model = model
        self.vocab_size = model.vocab_size
        self.lm_head = nn.Linear(model.hidden_size, model.vocab_size, bias=False, dtype=torch.float16)
        self.lm_head.weight.requires_grad_(False)
        if tie_word_embeddings:
            self.lm_head.weight = self.model.embed_tokens.weight

    @classmethod
    def from_config(cls, config, group_size: int):
        return cls(QuantLlamaModel.from_config(config, group_size), tie_word_embeddings=bool(getattr(config, "tie_word_embeddings", False)))

    def fuse_decode(self):
        self.model.fuse_decode()
        return self

    def fuse_prefill(self):
        self.model.fuse_prefill()
        return self

    def fuse_verify(self):
        self.model.fuse_verify()
        return self

    def unfuse_verify(self):
        self.model.unfuse_verify()
        return self

    def fuse_shared(self):
        self.model.fuse_shared()
        return self

    def unfuse_shared(self):
        self.model.unfuse_shared()
        return self

    @property
    def shared_fused(self) -> bool:
        return self.model.shared_fused

    def fuse_qkv(self):
        self.model.fuse_qkv()
        return self

    def forward(self, input_ids: torch.Tensor, cache, step_or_start, all_rows: bool = False) -> torch.Tensor:
        return F.linear(self.model(input_ids, cache, step_or_start, all_rows), self.lm_head.weight)

    def new_cache(self, num_blocks: int, block_size: int = 16, dtype=torch.float16) -> PagedKVCache:
        """A PagedKVCache of this model's layer count and head shape on its device."""
        attn = self.model.layers[0].self_attn
        return PagedKVCache(len(self.model.layers), num_blocks, attn.num_key_value_heads, attn.head_dim, block_size,
                            device=self.lm_head.weight.device, dtype=dtype)

    @torch.no_grad()
    def generate(self, prompts: Sequence[Sequence[int]], max_new_tokens: int, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                 generator: Optional[torch.Generator] = None, eos_token_id: Optional[int] = None, cache: Optional[PagedKVCache] = None,
                 block_size: int = 16, dtype=torch.float16, lora=None, adapters: Optional[Sequence[Optional[int]]] = None,
                 device_loop: bool = False, stop: Optional[Sequence[Sequence[int]]] = None,
                 stop_token_ids: Optional[Sequence[int]] = None, min_new_tokens: int = 0, n: int = 1, logprobs: Optional[int] = None,
                 draft_len: int = 0, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                 frequency_penalty: float = 0.0) -> List[List[int]]:
        """Generate up to `max_new_tokens` tokens for every prompt (token lists of any lengths) -> the generated ids per prompt, the
        eos_token_id that ends a sequence included.

        Every forward pass is followed by ops.sample_tokens with u = torch.rand(rows, generator=generator) -- temperature 0 is greedy --
        and the sampled ids feed the next step's embedding without leaving the device; they are read back once per pass for the
        bookkeeping (PagedKVCache.step is host-side anyway).  A sequence that emits eos_token_id or reaches its budget leaves the batch
        and its blocks are freed at once.  `cache`: a PagedKVCache to run in (it may hold other sequences); default: a new one with room
        for everything (`block_size`, `dtype`).  A prompt is admitted once the free blocks cover its whole budget on top of what the
        running sequences may still take, so the pool never runs out mid-sequence; when it cannot hold all prompts at once the rest wait,
        in order, for blocks to come free.  Newly admitted prompts are prefilled in one packed step of their own and the running rows
        decode in another: a sequence's tokens do not depend on what else was in the batch.  The random draws do: one torch.rand per pass.

        device_loop=True hands the prompts to a DecodeLoop (qqq_amd/serve.py) of min(len(prompts), 64) rows, sized for the longest budget
        rounded up to a block: the decode steps replay from one captured graph and the host syncs once per several tokens.  Greedy tokens
        are the same; the random draws are the loop's (one torch.rand(rows, u_stride) per u_stride steps).

        draft_len=K > 0 (with device_loop=True, on a model with fuse_prefill() or fuse_verify()) makes that loop a SpecDecodeLoop: K tokens drafted by
        n-gram lookup ride behind every row's last token and a replay emits 1 ... K + 1 tokens per row.  The output distribution is
        unchanged; the tokens under a seed differ (K + 1 variates per row and step), greedy tokens are the same up to near-ties of the
        logits.  Every sequence needs K more keys of the pool.

        repetition_penalty (transformers' rule: a seen token's logit l becomes l / r if l > 0, else l * r; over prompt and output),
        presence_penalty and frequency_penalty (vLLM's: l - frequency * c - presence for a token emitted c > 0 times; over the output
        alone) act on every pass's logits before temperature, top-k and top-p, through ops.penalize_logits on all three paths (the device
        loops are then built with penalties=True).  1, 0 and 0 mean none, and then nothing of it runs.

        n=N > 1 (parallel sampling) returns per prompt a list of N completions.  A prompt is prefilled once; its N first tokens are N
        sampler draws from the one last-position logits row (repeated, and penalised when penalties are on), PagedKVCache.fork makes the
        siblings that go on, and from then on each is an ordinary row with its own variates, history, penalties, eos and budget.  The
        siblings share the prompt's full blocks until the last of them ends, so a prompt of L keys and a budget of B blocks takes
        B + (N - 1) * (B - L // block_size) blocks in place of N * B.  The draws: one torch.rand of (admitted prompts * N) per prefill
        pass, then as for n = 1 one per decode pass over the running rows; equal seeds give equal tokens.  Siblings are adjacent in every
        step, so a model with fuse_shared() reads their common keys once per pack of rows (the tokens are the same either way).
        device_loop=True builds the DecodeLoop with family=N; n > 1 with draft_len > 0 raises (there is no shared verify kernel).
        n=1 is the call described above, draw for draw.

        logprobs=k (0 <= k <= 32; None: off, and then nothing of it runs) makes the call return (tokens, records): `records` mirrors the
        nesting of `tokens` and holds per completion a TokenLogprobs of CPU tensors with one entry per emitted token, the eos included
        -- the token's log-probability and rank and the k most probable tokens with their log-probabilities, from ops.topk_logprobs
        behind every ops.sample_tokens (the first token's from the prefill logits; for n > 1 from the repeated rows).  The values are
        those of the logits row the sampler drew from: AFTER ops.penalize_logits when penalties are on, BEFORE temperature, top-k and
        top-p -- the model's distribution, not the truncated one the draw was made from.  The tokens are the same as without logprobs,
        draw for draw; the per-pass results stay on the device until the call returns (no further host sync per pass).
        device_loop=True builds the DecodeLoop with logprobs=k.  logprobs with draft_len > 0 raises: the speculative loop emits several
        tokens per row and step.

        stop, stop_token_ids, min_new_tokens (None, None, 0: off, and then nothing of it runs) are the further ways a completion -- what
        the call returns for one prompt or sibling -- ends.  stop_token_ids (at most 32 ids) are further eos ids: drawing one ends the
        completion and the token is included.  stop (at most 32 sequences of 1 ... 32 token ids; encode stop strings first): once the
        completion ends in one of them it ends and is cut IN FRONT of the match (vLLM's `stop` without include_stop_str_in_output); the
        match lies in the completion alone, never in the prompt, the earliest end wins and at one end eos_token_id and the stop ids go
        before a sequence (a completion that ends in its eos keeps it, also where a stop sequence ends in the same token), then the
        sequence given first.  min_new_tokens=M: while the completion has fewer than M tokens, eos_token_id and every stop id have
        their logit set to -inf by ops.ban_tokens in the row the sampler draws from -- after the penalties, before temperature, top-k and
        top-p, so logprobs=k records show the banned row -- and no stop sequence is tested at a length below M; the cut may still leave
        fewer than M tokens, as in vLLM, and the budget max_new_tokens wins over M.  logprobs records are cut like their tokens.  On the
        host path the matching is plain Python in the bookkeeping; device_loop=True builds the loop with stops=True, whose captured
        step runs ops.ban_tokens and ops.stop_check (no host sync per token); a speculative step that emits several tokens is checked at
        every new length in order, and tokens behind a match are dropped.

        lora=bank, adapters=[slot or None per prompt] (None, None: off, and then nothing of it runs): every prompt is served through the
        adapter in its slot of the LoraBank (qqq_amd/lora.py) -- ops.lora_add behind every targeted projection, the slot of every token of
        a pass in PagedStep.lora -- and a prompt with None through the base model.  The adapters of a batch are mixed per token and a row's
        result depends on its own adapter alone, so a prompt's tokens are those it gets when it is run alone with its adapter.  n > 1:
        the siblings inherit their prompt's slot.  device_loop=True builds the loop with lora=bank: its captured step holds the rows' slots
        in device memory, one capture serves every mix of adapters, and bank.load() / unload() between calls need no new capture."""
        n, draft_len = int(n), int(draft_len)
        if n < 1:
            raise ValueError(f"generate: n={n} must be at least 1")
        if logprobs is not None:
            logprobs = int(logprobs)
            if logprobs < 0 or logprobs > 32 or logprobs > self.lm_head.weight.shape[0]:
                raise ValueError(f"generate: logprobs={logprobs} outside [0, min(32, vocab)]")
            if draft_len > 0:
                raise ValueError(f"generate: logprobs={logprobs} cannot be combined with draft_len={draft_len} (the speculative loop keeps "
                                 f"no records)")
        if n > 1 and draft_len > 0:
            raise ValueError(f"generate: n={n} > 1 cannot be combined with draft_len={draft_len} (speculative steps have no shared-prefix kernel)")
        if draft_len < 0 or (draft_len > 0 and not device_loop):
            raise ValueError(f"generate: draft_len={draft_len} must be 0, or positive together with device_loop=True")
        req = Request("generate", self.lm_head.weight.shape[0], temperature, top_k, top_p, generator, eos_token_id, repetition_penalty,
                      presence_penalty, frequency_penalty, stop, stop_token_ids, min_new_tokens, n, logprobs, lora=lora, adapters=adapters)
        return self._generate(req, prompts, max_new_tokens, temperature, top_k, top_p, generator, eos_token_id, cache, block_size, dtype,
                              device_loop, draft_len)

    def _generate(self, req, prompts, max_new_tokens, temperature, top_k, top_p, generator, eos_token_id, cache, block_size, dtype,
                  device_loop, draft_len):
        """generate() behind its keyword checks, for the request object `req` (a GuidedRequest: generate_guided's)"""
        n = req.n
        prompts, out = req.begin(prompts)  # out, per sibling: prompt i's are i * n ... i * n + n - 1
        if max_new_tokens < 1 or not prompts:
            return req.result()
        dev = self.lm_head.weight.device
        bs = cache.block_size if cache is not None else block_size
        keys = [len(p) + max_new_tokens - 1 + draft_len for p in prompts]
        need = [-(-k // bs) for k in keys]
        fam_need = [req.family_blocks(len(p), k, bs) for p, k in zip(prompts, keys)]
        if cache is None:
            cache = self.new_cache(sum(fam_need), block_size, dtype)
        if device_loop:  # the classes are looked up in qqq_amd.serve at the call
            build, call = req.loop_keywords()
            rows, max_len = max(1, min(len(prompts), 64 // n)) * n, max(need) * cache.block_size
            if isinstance(req, GuidedRequest):  # capacities rounded up from the call's automaton: powers of two, at least 64
                room = lambda count: max(64, 1 << (count - 1).bit_length())  # noqa: E731
                loop = serve.GuidedDecodeLoop(self, cache, rows=rows, max_len=max_len, fsm_states=room(req.fsm.n_states),
                                              fsm_edges=room(req.fsm.n_edges), **build)
                return loop.generate_guided(prompts, req._given, max_new_tokens, temperature, top_k, top_p, generator, eos_token_id, **call)
            loop = (serve.SpecDecodeLoop(self, cache, rows=rows, max_len=max_len, draft_len=draft_len, **build) if draft_len else
                    serve.DecodeLoop(self, cache, rows=rows, max_len=max_len, **build))
            return loop.generate(prompts, max_new_tokens, temperature, top_k, top_p, generator, eos_token_id, **call)
        tag = object()  # sequence ids no other user of the cache can hold
        sid = lambda i: (tag, i)  # noqa: E731
        waiting, running = deque(range(len(prompts))), []  # prompts that wait; siblings that run (i * n + j)
        cur = None  # int64 [len(running)] on the device: the running sequences' last tokens
        workspace = torch.zeros(len(out) * self.lm_head.weight.shape[0], dtype=torch.int32, device=dev) if req.penalised else None

        def settle(seqs, toks, fork=False):
            """record a pass's tokens; -> (the sequences that go on, their tokens of the pass).  After a prefill pass with n > 1 (`fork`)
            only sibling 0 of a prompt exists yet: the others that go on are forked from it before it is freed, if it ends."""
            alive, rows, done = [], [], []
            for row, (i, t) in enumerate(zip(seqs, toks.tolist())):
                if req.receive(i, t, max_new_tokens):
                    if not fork or i % n == 0:
                        done.append(i)
                else:
                    if fork and i % n:
                        cache.fork(sid(i - i % n), sid(i))
                    alive.append(i)
                    rows.append(row)
            for i in done:
                cache.free(sid(i))
            return alive, toks if len(rows) == toks.shape[0] else toks[torch.tensor(rows, dtype=torch.int64, device=toks.device)]

        try:
            while waiting or running:
                if running:
                    step = cache.step([sid(i) for i in running], [1] * len(running))
                    logits = self(cur, cache, req.with_adapters(step, [i // n for i in running], step.counts))
                    toks = req.sample(logits, running, workspace)
                    running, cur = settle(running, toks)
                new = []
                owed = sum(need[i // n] - len(cache.blocks(sid(i))) for i in running)  # what the running sequences may still take
                while waiting and fam_need[waiting[0]] <= cache.free_blocks - owed:
                    i = waiting.popleft()
                    cache.add(sid(i * n))
                    owed += fam_need[i]
                    new.append(i)
                if not new:
                    if not running and waiting:
                        raise RuntimeError(f"generate: the pool's {cache.free_blocks} free blocks cannot hold a prompt that needs "
                                           f"{fam_need[waiting[0]]} (prompt and budget)")
                    continue
                ids = torch.tensor([t for i in new for t in prompts[i]], dtype=torch.int64, device=dev)
                born = [i * n + j for i in new for j in range(n)]
                step = cache.step([sid(i * n) for i in new], [len(prompts[i]) for i in new])
                logits = self(ids, cache, req.with_adapters(step, new, step.counts))
                toks = req.sample(logits, born, workspace)
                alive, first = settle(born, toks, fork=n > 1)
                cur = first if not running else torch.cat([cur, first])
                running = running + alive
        except BaseException:  # leave the caller's pool as it was found
            for i in range(len(out)):
                try:
                    cache.free(sid(i))
                except KeyError:  # ended, or never admitted
                    pass
            raise
        return req.result()

    @torch.no_grad()
    def generate_guided(self, prompts: Sequence[Sequence[int]], fsm, max_new_tokens: int, temperature: float = 0.0, top_k: int = 0,
                        top_p: float = 1.0, generator: Optional[torch.Generator] = None, eos_token_id: Optional[int] = None,
                        cache: Optional[PagedKVCache] = None, block_size: int = 16, dtype=torch.float16, device_loop: bool = False,
                        stop: Optional[Sequence[Sequence[int]]] = None, stop_token_ids: Optional[Sequence[int]] = None,
                        min_new_tokens: int = 0, n: int = 1, logprobs: Optional[int] = None, repetition_penalty: float = 1.0,
                        presence_penalty: float = 0.0, frequency_penalty: float = 0.0):
        """generate() with every completion held to a token automaton (qqq_amd/guided.py): `fsm` is one TokenFSM for all prompts, or a
        sequence with one entry per prompt (None: that prompt is unconstrained).  Returns what generate() returns; every other keyword
        means what it means there.

        In front of every draw ops.fsm_mask sets the logit of every token the completion's state has no edge for to -inf -- the row's
        eos_token_id stays drawable in an accepting state -- and the state then moves on over the token drawn.  The mask sits behind
        the penalties and the minimum-length ban, in front of temperature, top-k and top-p, so logprobs=k records show the masked row as
        they show the banned one.  A completion that reaches a terminal state (one without edges: the end of a choice nothing extends)
        ends there, with no eos; in an accepting state with edges it ends when it draws its eos; the budget, stop and stop_token_ids
        end it as in generate().  On the host path the states are plain Python in the bookkeeping (GuidedRequest); device_loop=True
        builds a GuidedDecodeLoop whose captured step runs ops.fsm_mask and ops.fsm_advance over the automaton in device memory, with
        capacities rounded up from this call's automaton: no token is read on the host between two syncs.

        A completion can leave its automaton only where every allowed logit was -inf or NaN (the ban of a minimum length in a state
        that allows nothing else, a model that overflowed): the call then raises RuntimeError, after the pool is left as it was found.
        There is no draft_len: a speculative step draws several tokens from logits computed before any of them is known, so its rows
        cannot be masked by the state behind the token in front -- guided decoding and SpecDecodeLoop do not combine."""
        n = int(n)
        if n < 1:
            raise ValueError(f"generate_guided: n={n} must be at least 1")
        if logprobs is not None:
            logprobs = int(logprobs)
            if logprobs < 0 or logprobs > 32 or logprobs > self.lm_head.weight.shape[0]:
                raise ValueError(f"generate_guided: logprobs={logprobs} outside [0, min(32, vocab)]")
        req = GuidedRequest(fsm, "generate_guided", self.lm_head.weight.shape[0], temperature, top_k, top_p, generator, eos_token_id,
                            repetition_penalty, presence_penalty, frequency_penalty, stop, stop_token_ids, min_new_tokens, n, logprobs)
        result = self._generate(req, prompts, max_new_tokens, temperature, top_k, top_p, generator, eos_token_id, cache, block_size, dtype,
                                device_loop, 0)
        if not device_loop:  # (the loop has raised for its own request)
            req.check()
        return result

    def beam_search(self, prompts: Sequence[Sequence[int]], max_new_tokens: int, num_beams: int = 4, length_penalty: float = 1.0,
                    early_stopping: bool = False, eos_token_id: Optional[int] = None, num_return_sequences: int = 1,
                    cache: Optional[PagedKVCache] = None, block_size: int = 16, dtype=torch.float16):
        """Beam search with `num_beams` beams (1 ... 16) for every prompt -> per prompt a list of `num_return_sequences` BeamHypothesis
        (tokens, score, logprob), best first.  The rules are transformers' (model.generate(num_beams=...), no sampling).

        One packed prefill of the admitted prompts, then one pass per token over all beams of all running prompts (row p * B + b).
        ops.beam_step runs behind every pass: each live beam's 2B most probable tokens, the beam's summed log-probability added in f32, a
        prompt's candidates merged and ordered, the first 2B kept; the first B of them that are not eos are the next beams, and their
        tokens feed the next pass without leaving the device.  One read-back per pass brings the candidates and the parents for the
        bookkeeping, and PagedKVCache.reorder re-points the beams' blocks once per pass: full blocks by reference, the partial blocks
        of a parent taken several times through one ops.copy_blocks launch.

        A candidate whose token is eos_token_id among the first B of its pass is a finished hypothesis and keeps its eos; at the budget
        max_new_tokens the live beams finish as they are.  score = logprob / len(tokens) ** length_penalty, the eos counted; the B best
        per prompt are kept.  early_stopping=True ends a prompt once B are held; False ends it when B are held and the best live beam's
        logprob / its length ** length_penalty is not above the worst held score (transformers' default heuristic).  A prompt that is
        done leaves the batch and frees its blocks; the call ends when every prompt is done.  num_beams=1 gives greedy generate's tokens.

        `cache`: a PagedKVCache to run in (other sequences in it are left alone); default: a new one with room for everything.  A prompt
        of L tokens is admitted once the free blocks cover own + (num_beams - 1) * (own - L // block_size), own = ceil((L +
        max_new_tokens - 1) / block_size), on top of what the running prompts may still take (beam.blocks_needed: the prompt's full
        blocks are held once, everything else once per beam); prompts that do not fit wait in order, and one that can never fit raises
        RuntimeError ("cannot hold a prompt").  Newly admitted prompts are prefilled in a pass of their own.  fuse_prefill(),
        fuse_decode() and the cache dtype are honoured as in generate.  Sampling inside the beam, penalties, stop sequences, logprobs
        records, device_loop, draft_len and n are not part of this call."""
        from . import beam as _beam

        return _beam.beam_search(self, prompts, max_new_tokens, num_beams=num_beams, length_penalty=length_penalty,
                                 early_stopping=early_stopping, eos_token_id=eos_token_id, num_return_sequences=num_return_sequences,
                                 cache=cache, block_size=block_size, dtype=dtype)

    def score(self, sequences: Sequence[Sequence[int]], cache: Optional[PagedKVCache] = None, chunk_tokens: int = 2048, block_size: int = 16,
              dtype=torch.float16, return_greedy: bool = False):
        """Per-token log-probabilities log p(seq[t + 1] | seq[:t + 1]) of every sequence, f32 [len - 1] each (with return_greedy also the
        argmax ids), in chunks of `chunk_tokens` tokens over a paged cache through ops.token_logprobs: qqq_amd/score.py::score."""
        from . import score as _score

        return _score.score(self, sequences, cache=cache, chunk_tokens=chunk_tokens, block_size=block_size, dtype=dtype,
                            return_greedy=return_greedy)

    def loglikelihood(self, requests, **score_kw):
        """[(sum of the continuation's log-probs, is_greedy)] for (context_ids, continuation_ids) requests, the shape of lm-eval's
        loglikelihood: qqq_amd/score.py::loglikelihood."""
        from . import score as _score

        return _score.loglikelihood(self, requests, **score_kw)

    def perplexity(self, token_ids, seqlen: int = 2048, **score_kw) -> float:
        """Perplexity over numel // seqlen disjoint windows by the convention of the reference's examples/eval_model.py (per window the
        mean NLL of its seqlen - 1 targets times seqlen; exp(sum / (nsamples * seqlen))): qqq_amd/score.py::perplexity."""
        from . import score as _score

        return _score.perplexity(self, token_ids, seqlen, **score_kw)


__all__ = ["QuantLlamaModel", "QuantLlamaForCausalLM"]
