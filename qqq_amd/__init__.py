"""qqq_amd -- MI355X-native (gfx950) W4A8 GEMM behind QQQ's `qqq_gemm` operator.

Public surface (mirrors the reference's hot path, HandH1998/QQQ):
    qqq_gemm(A, B, C, D, s1, s2, s3, workspace, thread_k, thread_n, sms, max_par)   # QQQ._CUDA.qqq_gemm
    mul(...)                                                                       # qlinear_marlin.mul
    QuantLinear                                                                    # qlinear_marlin.QuantLinear
    marlin_qqq_gemm(...)                                                           # vLLM-style wrapper
    dynamic_quant(x)                                                               # fused per-token int8 quant
    quantlinear_forward(x, B, C, s2, s3, workspace, bias)                          # QuantLinear.forward, one call
    expand_int8(B, s_group) / QuantLinear.expand_for_prefill()                     # opt-in load-time int8 expansion
    rmsnorm_quant(x, weight, eps, residual) / silu_mul_quant(gate, up)              # decoder activations, produced already int8-quantised
    QuantLinear.forward_int8(xq, s1), QuantRMSNorm, QuantLlamaMLP                     # the layer on pre-quantised input; qqq_amd/blocks.py
    rope_qkv(q, k, v, cos, sin, pos, k_cache, v_cache)                              # RoPE on q/k + static KV-cache write, one launch
    decode_attention(q_out, k_cache, v_cache, pos, scale)                           # split-K decode attention over the cache, output int8-quantised
    rope_qkv_kv8(..., k_cache, v_cache, k_scale, v_scale) / decode_attention_kv8(...)  # the same two over an int8 KV cache (KVCache(dtype=torch.int8))
    rope_qkv_paged(..., pos, slots, k_pool, v_pool) / decode_attention_paged(q_out, k_pool, v_pool, block_table, pos, scale)  # the same two
    rope_qkv_paged_kv8(...) / decode_attention_paged_kv8(...)                       # over block pools (fp16 / int8) through slots and a block table
    prefill_attention_paged(q_out, k_pool, v_pool, block_table, cu_tokens, start_pos, scale) / prefill_attention_paged_kv8(...)  # ragged causal
                                                                                    # prefill attention over the block pools, output int8-quantised
    verify_attention_paged(q_out, k_pool, v_pool, block_table, start, tokens, scale) / verify_attention_paged_kv8(...)  # a verify chunk of
                                                                                    # `tokens` tokens per row through the decode kernel, bit for bit
    decode_attention_paged_shared(q_out, k_pool, v_pool, block_table, pos, family, shared, pack, scale) / ..._kv8(...)  # decode attention of
                                                                                    # forked siblings: shared keys read once per pack, bit for bit
    rope_qkv_norm(q, k, v, q_weight, k_weight, eps, cos, sin, pos, k_cache, v_cache) / rope_qkv_norm_kv8(...) / rope_qkv_norm_paged(...) /
    rope_qkv_norm_paged_kv8(...)                                                    # the four RoPE / cache-write ops with Qwen3's per-head
                                                                                    # q_norm / k_norm in front of the rotation, still one launch
    KVCache, QuantLlamaAttention, QuantLlamaDecoderLayer                            # attention and the whole layer; qqq_amd/attention.py
    PagedKVCache, PagedStep                                                        # block pools + host-side allocator; qqq_amd/paged.py
    sample_tokens(logits, temperature, top_k, top_p, u)                             # temperature / top-k / top-p / draw for a batch, one launch
    QuantLlamaModel, QuantLlamaForCausalLM                                         # the whole model and generate(); qqq_amd/model.py
    sample_advance(logits, ..., u, tick, ids, pos, slots, block_table, remaining, eos, out, n_out, block_size)  # sample_tokens + the decode
                                                                                    # loop's per-row bookkeeping on the device, one launch
    DecodeLoop(lm, cache, rows, max_len)                                            # device-resident decode loop, one graph per step; qqq_amd/serve.py
    spec_advance(logits, ..., u, tick, ids, pos, slots, start, block_table, remaining, eos, hist, hist_len, n_out, n_acc, block_size, ngram_max)
                                                                                    # draft_len + 1 draws per row, accept rule, n-gram drafter
    SpecDecodeLoop(lm, cache, rows, max_len, draft_len=4), ngram_draft              # speculative decode loop, 1 ... draft_len + 1 tokens per replay
    penalize_logits(logits, ids, pos, seen, n_prompt, repetition, presence, frequency)  # penalties from each row's history, in place, before a sampler
    token_logprobs(logits, targets, return_argmax=True)                             # a target's log-probability and the argmax per logit row, one launch
    QuantLlamaForCausalLM.score / loglikelihood / perplexity, pack_steps            # scoring text over the paged cache; qqq_amd/score.py
    topk_logprobs(logits, tokens=None, k=0) / topk_logprobs_step(...)               # a token's log-probability and rank and the k most probable
                                                                                    # tokens per logit row, one launch; generate(logprobs=k)
    ban_tokens(logits, n_out, min_new, eos, ban_ids, base) / stop_check(tokens, base, first, n_out, stop_ids, stop_len, ...)
                                                                                    # the minimum length in front of a sampler, stop sequences and
                                                                                    # stop token ids behind a loop's step; generate(stop=, ...)
    beam_step(logits, cum, live, num_beams, eos) / copy_blocks(pools, src, dst, block_bytes, num_blocks)
                                                                                    # a beam-search step behind a pass's logits, one launch; the
                                                                                    # block copies of PagedKVCache.reorder, one launch
    QuantLlamaForCausalLM.beam_search(prompts, max_new_tokens, num_beams=4, ...), BeamHypothesis   # beam search; qqq_amd/beam.py
    fsm_mask(logits, state, fsm_tensors, eos, remaining) / fsm_advance(out, n_out, n_fsm, state, fsm_tensors, ids, pos, slots, remaining, eos)
                                                                                    # guided decoding: a token automaton in device memory masks
                                                                                    # the row in front of a sampler and advances behind it
    TokenFSM, QuantLlamaForCausalLM.generate_guided(prompts, fsm, max_new_tokens, ...), GuidedDecodeLoop   # qqq_amd/guided.py, serve.py
    lora_add(y, xq, s1, A, B, scale, slot, part_cols)                               # batched LoRA beside the GEMM: every row adds its own
                                                                                    # adapter's low-rank product, its slot read on the device
    LoraBank(lm, slots, rank), LoraStep, generate(..., lora=bank, adapters=[...])   # multi-LoRA serving; qqq_amd/lora.py
"""
from .ops import (  # noqa: F401
    ban_tokens,
    beam_step,
    copy_blocks,
    decode_attention,
    decode_attention_kv8,
    decode_attention_paged,
    decode_attention_paged_kv8,
    dynamic_quant,
    expand_int8,
    fsm_advance,
    fsm_mask,
    lora_add,
    marlin_qqq_gemm,
    mul,
    penalize_logits,
    prefill_attention_paged,
    prefill_attention_paged_kv8,
    qqq_gemm,
    qqq_gemm_bias,
    qqq_gemm_ex,
    qqq_gemm_w8,
    quantlinear_forward,
    rmsnorm_quant,
    rope_qkv,
    rope_qkv_kv8,
    rope_qkv_paged,
    rope_qkv_paged_kv8,
    rope_qkv_norm,
    rope_qkv_norm_kv8,
    rope_qkv_norm_paged,
    rope_qkv_norm_paged_kv8,
    sample_advance,
    sample_tokens,
    silu_mul_quant,
    spec_advance,
    stop_check,
    token_logprobs,
    topk_logprobs,
    topk_logprobs_step,
    verify_attention_paged,
    verify_attention_paged_kv8,
    decode_attention_paged_shared,
    decode_attention_paged_shared_kv8,
    decode_attention_shared_plan,
)
from .qlinear import QuantLinear, fuse_quant_linears  # noqa: F401
from .blocks import QuantLlamaMLP, QuantRMSNorm  # noqa: F401
from .attention import KVCache, QuantLlamaAttention, QuantLlamaDecoderLayer  # noqa: F401
from .paged import PagedKVCache, PagedStep  # noqa: F401
from .request import TokenLogprobs  # noqa: F401
from .model import QuantLlamaForCausalLM, QuantLlamaModel  # noqa: F401
from .serve import DecodeLoop, GuidedDecodeLoop, SpecDecodeLoop, ngram_draft  # noqa: F401
from .guided import TokenFSM  # noqa: F401
from .lora import LoraBank, LoraStep  # noqa: F401
from .score import pack_steps  # noqa: F401
from .beam import BeamHypothesis  # noqa: F401

__all__ = ["qqq_gemm", "qqq_gemm_bias", "qqq_gemm_ex", "qqq_gemm_w8", "expand_int8", "mul", "marlin_qqq_gemm", "dynamic_quant", "quantlinear_forward",
           "rmsnorm_quant", "silu_mul_quant", "QuantLinear", "fuse_quant_linears", "QuantRMSNorm", "QuantLlamaMLP",
           "rope_qkv", "decode_attention", "rope_qkv_kv8", "decode_attention_kv8", "rope_qkv_paged",
           "decode_attention_paged", "rope_qkv_paged_kv8", "decode_attention_paged_kv8", "prefill_attention_paged",
           "prefill_attention_paged_kv8", "PagedKVCache", "PagedStep", "KVCache", "QuantLlamaAttention", "QuantLlamaDecoderLayer",
           "sample_tokens", "QuantLlamaModel", "QuantLlamaForCausalLM", "sample_advance", "DecodeLoop", "token_logprobs", "pack_steps",
           "spec_advance", "SpecDecodeLoop", "ngram_draft", "verify_attention_paged", "verify_attention_paged_kv8", "penalize_logits",
           "decode_attention_paged_shared", "decode_attention_paged_shared_kv8", "decode_attention_shared_plan",
           "topk_logprobs", "topk_logprobs_step", "TokenLogprobs", "ban_tokens", "stop_check",
           "beam_step", "copy_blocks", "BeamHypothesis", "fsm_mask", "fsm_advance", "TokenFSM", "GuidedDecodeLoop",
           "lora_add", "LoraBank", "LoraStep", "rope_qkv_norm", "rope_qkv_norm_kv8", "rope_qkv_norm_paged", "rope_qkv_norm_paged_kv8"]
