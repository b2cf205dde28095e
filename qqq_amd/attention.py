"""The attention half of a Llama / Qwen2 decoder layer around QuantLinear, and the layer itself: the reference's
QuantizedLlamaAttention / QuantizedQwen2Attention and Quantized{Llama,Qwen2}DecoderLayer (QQQ/gptq/models/llama.py, qwen2.py).

    rope_tables       cos / sin tables [length, head_dim] as transformers' rotary embedding computes them (rope_type "default", "llama3")
    KVCache           static fp16 K / V per layer, [b, kvh, capacity, head_dim], allocated once: no history copy per step; opt-in
                      dtype=torch.int8: every head row as int8 codes and one f32 scale (rope_qkv_kv8 / decode_attention_kv8)
    PagedKVCache      (qqq_amd/paged.py) block pools [num_blocks, kvh, block_size, head_dim] with a host-side block allocator, fp16 or
                      int8: sequences of different lengths in one packed batch, blocks reused when a sequence finishes
    QuantLlamaAttention      q/k/v GEMMs on the int8 input of QuantRMSNorm -> rope_qkv (RoPE on q and k, k / v into the cache, one launch)
                             -> scaled_dot_product_attention -> dynamic_quant -> o_proj;  opt-in fuse_decode(): one-token steps take
                             decode_attention (split-K over the cache, output int8-quantised) in place of the last two
    QuantLlamaDecoderLayer   input_layernorm, self_attn, post_attention_layernorm (residual add fused), mlp, final residual add;
                             forward_chained() leaves that last add to the next layer's norm (qqq_amd/model.py)

The attention core is torch's scaled_dot_product_attention, as in the reference, unless fuse_decode() is on and the step has one token.

Paged cache: forward_int8(xq, s1, cache, step) with a PagedKVCache takes a PagedStep (cache.step(seq_ids, counts)) in place of the start
position and xq [m, hidden] with the sequences' tokens packed in order.  rope_qkv_paged(_kv8) writes all m tokens in one launch; a step of
one token per sequence runs decode_attention_paged(_kv8) through the step's block table, whatever fuse_decode() says; any other step runs
scaled_dot_product_attention per sequence over PagedKVCache.gather (a contiguous copy), or, after the opt-in fuse_prefill(),
prefill_attention_paged(_kv8): one ragged causal attention over the whole packed batch that reads the pool in place and writes o_proj's
input already int8-quantised.  After the opt-in fuse_verify() a step that feeds every sequence the same 2 ... 16 tokens (a speculative decode
step's chunk) runs verify_attention_paged(_kv8): the decode kernel's split over keys, every token bit for bit its decode step.
Qwen3 (qk_norm=True): a per-head RMSNorm of q and k between the projections and RoPE; every rope_qkv* call above is then its
rope_qkv_norm* counterpart, the norm inside the same launch (include_ops/qqq_amd_qknorm.h).
Parameter and buffer names are the reference's, so the layers' state-dicts load unchanged; the rope tables, the fused q|k|v copy of
fuse_qkv() and the fuse_decode() / fuse_prefill() / fuse_verify() / fuse_shared() flags are not part of them.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .blocks import QuantLlamaMLP, QuantRMSNorm, _no_lora, forward_int8_lora, lora_add_slices
from .paged import PagedKVCache, PagedStep
from .qlinear import QuantLinear, fuse_quant_linears


def rope_inv_freq(head_dim: int, rope_theta: float = 10000.0, rope_scaling: Optional[dict] = None):
    """(inv_freq fp32 [head_dim / 2] on the CPU, attention_scaling) of transformers' rope initialisers for rope_type "default" (Llama-2,
    Llama-3, Qwen2) and "llama3" (Llama-3.1 / 3.2).  `rope_scaling` is a transformers rope dict ("rope_type" or the older "type" key) or
    None; every other rope type, and a partial rotary factor, raises NotImplementedError."""
    sc = dict(rope_scaling or {})
    rope_type = sc.get("rope_type", sc.get("type", "default")) or "default"
    if rope_type not in ("default", "llama3"):
        raise NotImplementedError(f"rope_type {rope_type!r} is not supported (only 'default' and 'llama3')")
    if float(sc.get("partial_rotary_factor", 1.0)) != 1.0:
        raise NotImplementedError("a partial rotary factor is not supported")
    base, dim = float(sc.get("rope_theta", rope_theta)), int(head_dim)
    inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.int64).to(dtype=torch.float) / dim))
    if rope_type == "llama3":
        factor, low, high = sc["factor"], sc["low_freq_factor"], sc["high_freq_factor"]
        old_len = sc["original_max_position_embeddings"]
        low_wavelen, high_wavelen = old_len / low, old_len / high
        wavelen = 2 * math.pi / inv_freq
        inv_freq_llama = torch.where(wavelen > low_wavelen, inv_freq / factor, inv_freq)
        smooth = (old_len / wavelen - low) / (high - low)
        smoothed = (1 - smooth) * inv_freq_llama / factor + smooth * inv_freq_llama
        is_medium = ~(wavelen < high_wavelen) * ~(wavelen > low_wavelen)
        inv_freq = torch.where(is_medium, smoothed, inv_freq_llama)
    return inv_freq, 1.0


@torch.no_grad()
def rope_tables(inv_freq: torch.Tensor, attention_scaling: float, length: int, device, dtype=torch.float16):
    """(cos, sin) [length, 2 * inv_freq.numel()] for positions 0 ... length-1: transformers' rotary forward on `device` (fp32 freqs =
    inv_freq @ positions, emb = cat(freqs, freqs), cos = emb.cos() * attention_scaling, then cast to `dtype`)."""
    inv = inv_freq.to(device=device, dtype=torch.float)[None, :, None]
    positions = torch.arange(length, device=device)[None, None, :].float()
    freqs = (inv @ positions).transpose(1, 2)
    emb = torch.cat((freqs, freqs), dim=-1)
    return (emb.cos() * attention_scaling).to(dtype)[0], (emb.sin() * attention_scaling).to(dtype)[0]


class KVCache:
    """Static key / value cache of `num_layers` layers: k[layer], v[layer] of shape [batch, num_kv_heads, capacity, head_dim], allocated
    (zeroed) once, written in place by rope_qkv at each token's position.  In a KVCache every batch row is at the same position (no
    per-row lengths, no paging: that is PagedKVCache, qqq_amd/paged.py).

    dtype=torch.float16 (default): fp16 K and V, 4 * num_layers * batch * num_kv_heads * capacity * head_dim bytes.
    dtype=torch.int8: every head row is dynamic_quant of that fp16 row -- int8 codes in k / v plus one f32 scale per row in k_scale[layer],
    v_scale[layer] of shape [batch, num_kv_heads, capacity] -- written by rope_qkv_kv8 and read by decode_attention_kv8:
    2 * num_layers * batch * num_kv_heads * capacity * (head_dim + 4) bytes.  Any other dtype raises."""

    def __init__(self, num_layers: int, batch: int, num_kv_heads: int, head_dim: int, capacity: int, device=None, dtype=torch.float16):
        if dtype not in (torch.float16, torch.int8):
            raise ValueError(f"KVCache: dtype must be torch.float16 or torch.int8, not {dtype}")
        self.num_layers, self.batch, self.num_kv_heads, self.head_dim, self.capacity = num_layers, batch, num_kv_heads, head_dim, capacity
        self.dtype = dtype
        shape = (batch, num_kv_heads, capacity, head_dim)
        self.k = [torch.zeros(shape, dtype=dtype, device=device) for _ in range(num_layers)]
        self.v = [torch.zeros(shape, dtype=dtype, device=device) for _ in range(num_layers)]
        if dtype == torch.int8:
            self.k_scale = [torch.zeros(shape[:3], dtype=torch.float32, device=device) for _ in range(num_layers)]
            self.v_scale = [torch.zeros(shape[:3], dtype=torch.float32, device=device) for _ in range(num_layers)]
        # positions p of every batch row, [capacity, batch]: the s = 1 (decode) and b = 1 position vectors are views of it, no launch
        self._rep = torch.arange(capacity, device=device)[:, None].expand(capacity, batch).contiguous()

    @property
    def quantized(self) -> bool:
        return self.dtype == torch.int8

    @property
    def nbytes(self) -> int:
        rows = self.num_layers * self.batch * self.num_kv_heads * self.capacity
        return 2 * rows * (self.head_dim + 4) if self.quantized else 4 * rows * self.head_dim

    def positions(self, start: int, s: int) -> torch.Tensor:
        """int64 [batch * s] device positions start ... start+s-1 of every batch row (token bi * s + si)."""
        if s == 1 or self.batch == 1:
            return self._rep[start:start + s].reshape(-1)
        return self._rep[start:start + s, 0].repeat(self.batch)

    def dequant(self, layer: int, length: int):
        """(k, v) fp16 [batch, num_kv_heads, length, head_dim] of an int8 cache's first `length` slots: fp16(float(code) * scale), plain
        torch on the cache's device (CPU tensors too)."""
        if not self.quantized:
            raise RuntimeError("KVCache.dequant: the cache is not int8")
        return tuple((c[:, :, :length].float() * sc[:, :, :length, None]).half()
                     for c, sc in ((self.k[layer], self.k_scale[layer]), (self.v[layer], self.v_scale[layer])))


class _HeadNorm(nn.Module):
    """The holder of a Qwen3 q_norm / k_norm: `weight` fp16 [head_dim] (ones at construction) under transformers' state-dict name, and
    eps.  It has no forward: the norm runs inside the rope_qkv_norm* launch of the attention module that owns it."""

    def __init__(self, head_dim: int, eps: float):
        super().__init__()
        self.eps = float(eps)
        self.weight = nn.Parameter(torch.ones(head_dim, dtype=torch.float16), requires_grad=False)


def _drop_fused_qkv_on_load(module, *args, **kwargs):
    module._qkv = None  # a state-dict is being loaded: the fused q|k|v copy would be stale


class QuantLlamaAttention(nn.Module):
    """QuantizedLlamaAttention / QuantizedQwen2Attention (SDPA) with W4A8 QuantLinears and a static KV cache.

    forward_int8(xq, s1, cache, start): (xq int8 [b*s, hidden], s1 f32 [b*s, 1]) as QuantRMSNorm returns them, tokens at positions
    start ... start+s-1 (the same for every batch row) -> fp16 [b*s, hidden].  forward(x, cache, start) quantises its fp16 input first.
    With a PagedKVCache `start` is a PagedStep and xq [m, hidden] holds the sequences' tokens packed in order (see the module docstring).
    Llama: qkv_bias = o_bias = config.attention_bias;  Qwen2: qkv_bias=True, o_bias=False.
    Qwen3: qk_norm=True -- the module owns q_norm.weight and k_norm.weight (fp16 [head_dim], transformers' names), a per-head RMSNorm with
    eps = rms_norm_eps between the q / k projections and RoPE, and every RoPE / cache-write launch is its rope_qkv_norm* counterpart
    (the norm runs inside that launch).  Without qk_norm nothing of this is registered, allocated or run."""

    def __init__(self, hidden: int, num_heads: int, num_kv_heads: int, group_size: int, head_dim: Optional[int] = None,
                 qkv_bias: bool = False, o_bias: bool = False, rope_theta: float = 10000.0, rope_scaling: Optional[dict] = None,
                 layer_idx: int = 0, qk_norm: bool = False, rms_norm_eps: float = 1e-6):
        super().__init__()
        head_dim = head_dim or hidden // num_heads
        if qk_norm and head_dim not in (64, 128):
            raise ValueError(f"qk_norm needs head_dim 64 or 128, not {head_dim}")
        if num_heads % num_kv_heads:
            raise ValueError(f"num_heads {num_heads} must be a multiple of num_kv_heads {num_kv_heads}")
        if head_dim % 16 or head_dim > 256:
            raise ValueError(f"head_dim {head_dim} must be a multiple of 16, at most 256")
        self.hidden_size, self.num_heads, self.num_key_value_heads, self.head_dim = hidden, num_heads, num_kv_heads, head_dim
        self.layer_idx = layer_idx
        self.scaling = head_dim ** -0.5
        self.q_proj = QuantLinear(4, group_size, hidden, num_heads * head_dim, bias=qkv_bias)
        self.k_proj = QuantLinear(4, group_size, hidden, num_kv_heads * head_dim, bias=qkv_bias)
        self.v_proj = QuantLinear(4, group_size, hidden, num_kv_heads * head_dim, bias=qkv_bias)
        self.o_proj = QuantLinear(4, group_size, num_heads * head_dim, hidden, bias=o_bias)
        self.qk_norm = bool(qk_norm)
        if self.qk_norm:
            self.q_norm, self.k_norm = _HeadNorm(head_dim, rms_norm_eps), _HeadNorm(head_dim, rms_norm_eps)
        self.inv_freq, self.attention_scaling = rope_inv_freq(head_dim, rope_theta, rope_scaling)  # plain attributes: not in the state-dict
        self._cos = self._sin = None  # rope tables, built lazily up to the cache capacity on the module's device
        self._qkv = None  # fuse_qkv(): the fused q|k|v layer, kept outside the module tree (not in the state-dict)
        self._decode = False  # fuse_decode(): a plain flag (not in the state-dict; kept by load_state_dict and .to())
        self._prefill = False  # fuse_prefill(): the same kind of flag
        self._verify = False  # fuse_verify(): the same kind of flag
        self._shared = False  # fuse_shared(): the same kind of flag
        # a plain function: a bound method would make module -> hook -> module a reference cycle (see QuantLlamaMLP)
        self._register_load_state_dict_pre_hook(_drop_fused_qkv_on_load, with_module=True)

    def rope_tables(self, length: int):
        """(cos, sin) fp16 [>= length, head_dim] on the module's device, built on first need and regrown when a longer cache arrives."""
        dev = self.q_proj.B.device
        if self._cos is None or self._cos.shape[0] < length or self._cos.device != dev:
            self._cos, self._sin = rope_tables(self.inv_freq, self.attention_scaling, length, dev)
        return self._cos, self._sin

    @torch.no_grad()
    def fuse_qkv(self):
        """Opt-in: ONE GEMM for q, k and v (fuse_quant_linears: N = (h + 2 kvh) * head_dim), whose three column ranges feed rope_qkv in
        place.  Memory: a second copy of the three layers' weights, scales and bias.  state_dict(): unchanged.  Loading a state-dict drops
        the fused copy (the module then runs the three GEMMs until fuse_qkv() is called again); unfuse_qkv() releases it.  The fused layer
        follows later .to() / .cuda() moves of the module.  Returns self."""
        fused = fuse_quant_linears([self.q_proj, self.k_proj, self.v_proj])
        if all(p.W8 is not None for p in (self.q_proj, self.k_proj, self.v_proj)):
            fused.expand_for_prefill(per_channel=True)
        object.__setattr__(self, "_qkv", fused)  # a plain attribute: nn.Module would register it as a submodule
        return self

    def unfuse_qkv(self):
        """Release the fused q|k|v layer of fuse_qkv()."""
        self._qkv = None
        return self

    @property
    def qkv_fused(self) -> bool:
        return self._qkv is not None

    def fuse_decode(self):
        """Opt-in: a step of one token (s = 1) runs the split-K decode attention kernel over the cache (decode_attention), which writes
        o_proj's input already int8-quantised: two launches in place of scaled_dot_product_attention and dynamic_quant.  Prefill, chunks
        (s > 1) and head shapes the kernel does not take (head_dim other than 64 / 128, more than 8 query heads per KV head, h * head_dim
        above 16384) keep the SDPA path.  state_dict(): unchanged.  Returns self."""
        self._decode = True
        return self

    def unfuse_decode(self):
        """Back to scaled_dot_product_attention + dynamic_quant for every step."""
        self._decode = False
        return self

    @property
    def decode_fused(self) -> bool:
        return self._decode

    def fuse_prefill(self):
        """Opt-in: a step over a PagedKVCache that is not a decode step (a prompt, a chunk, chunks batched with decoding rows) runs
        prefill_attention_paged(_kv8) -- one ragged causal attention launch over the whole packed batch that reads K and V through the
        block table in place, and one that quantises its rows for o_proj -- in place of the per-sequence gather, scaled_dot_product_attention
        and dynamic_quant.  Decode steps and KVCache paths are unchanged.  state_dict(): unchanged.  Returns self."""
        self._prefill = True
        return self

    def unfuse_prefill(self):
        """Back to scaled_dot_product_attention over PagedKVCache.gather for paged steps of more than one token."""
        self._prefill = False
        return self

    @property
    def prefill_fused(self) -> bool:
        return self._prefill

    def fuse_verify(self):
        """Opt-in: a step over a PagedKVCache that feeds every sequence the same number T of tokens, 2 <= T <= 16 with (h / kvh) * T <= 64
        -- the chunk of a speculative decode step -- runs verify_attention_paged(_kv8): the decode kernel's split over keys with the
        chunk's queries in the padding of its operands, every token's row bit for bit the decode step's for that token.  Every other step
        goes where it goes without the flag (decode steps to the decode kernel, ragged or wider chunks to fuse_prefill()'s path or
        SDPA).  state_dict(): unchanged.  Returns self."""
        self._verify = True
        return self

    def unfuse_verify(self):
        """Uniform chunks go back to where every other chunk goes."""
        self._verify = False
        return self

    @property
    def verify_fused(self) -> bool:
        return self._verify

    def fuse_shared(self):
        """Opt-in: a decode step over a PagedKVCache in which adjacent sequences were forked from one prompt (PagedStep.family is set: the
        n completions of parallel sampling) runs decode_attention_paged_shared(_kv8) with pack = min(family_max, 64 // (h // kvh)): the
        splits inside a family's shared keys are read once per pack of rows, every row bit for bit the plain decode step's.  Every other
        step goes where it goes without the flag; without it a step with families runs the plain paged decode op over the aliased
        tables.  state_dict(): unchanged.  Returns self."""
        self._shared = True
        return self

    def unfuse_shared(self):
        """Decode steps with families go back to the plain paged decode op."""
        self._shared = False
        return self

    @property
    def shared_fused(self) -> bool:
        return self._shared

    def _verify_tokens(self, step: PagedStep) -> int:
        """T if fuse_verify() is set and `step` is a chunk the verify kernel takes (from the step's host lists alone), else 0."""
        if not self._verify or step.decode or step.start_pos is None or not step.counts:
            return 0
        t = step.counts[0]
        if t < 2 or t > 16 or (self.num_heads // self.num_key_value_heads) * t > 64 or any(c != t for c in step.counts):
            return 0
        return t

    def _decode_supported(self) -> bool:
        h, kvh, d = self.num_heads, self.num_key_value_heads, self.head_dim
        return d in (64, 128) and h // kvh <= 8 and h * d <= 16384

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse=recurse)
        if self._qkv is not None:
            self._qkv._apply(fn, recurse=recurse)
        return self

    def project_qkv(self, xq: torch.Tensor, s1: torch.Tensor, lora=None):
        """(q, k, v) fp16 token rows [b*s, h*d], [b*s, kvh*d], [b*s, kvh*d]: three views into one output after fuse_qkv().  `lora`: None, or
        the layer's LayerLora (qqq_amd/lora.py), whose adapters are added to the projections it holds."""
        pick = lora if lora is not None else _no_lora
        if self._qkv is not None:
            qkv = forward_int8_lora(self._qkv, xq, s1, pick("qkv"))
            nq, nk = self.num_heads * self.head_dim, self.num_key_value_heads * self.head_dim
            q, k, v = qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:]
            if lora is not None and pick("qkv") is None:  # part of the group is targeted: its columns of the fused output
                lora_add_slices(xq, s1, lora, (("q_proj", q), ("k_proj", k), ("v_proj", v)))
            return q, k, v
        return (forward_int8_lora(self.q_proj, xq, s1, pick("q_proj")), forward_int8_lora(self.k_proj, xq, s1, pick("k_proj")),
                forward_int8_lora(self.v_proj, xq, s1, pick("v_proj")))

    def attend(self, q_out: torch.Tensor, cache: KVCache, start: int) -> torch.Tensor:
        """scaled_dot_product_attention of q_out [b, h, s, d] over the cache slice [:, :, :start+s] -> fp16 [b, s, h*d]: causal for a
        prefill from 0, a bottom-right causal mask for a chunk at start > 0, no mask for one token.  An int8 cache is dequantised first
        (KVCache.dequant), so prefill attends to the quantised K / V that decode reads later."""
        b, h, s, d = q_out.shape
        if cache.quantized:
            kc, vc = cache.dequant(self.layer_idx, start + s)
        else:
            kc = cache.k[self.layer_idx][:, :, :start + s]
            vc = cache.v[self.layer_idx][:, :, :start + s]
        return self._sdpa(q_out, kc, vc, start)

    def _sdpa(self, q_out: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, start: int) -> torch.Tensor:
        """q_out [b, h, s, d] at positions start ... start+s-1 over keys 0 ... start+s-1 (kc, vc [b, kvh, start+s, d]) -> [b, s, h*d]"""
        b, h, s, d = q_out.shape
        mask = None
        if s > 1 and start > 0:
            mask = torch.ones((s, start + s), dtype=torch.bool, device=q_out.device).tril(diagonal=start)
        o = F.scaled_dot_product_attention(q_out, kc, vc, attn_mask=mask, is_causal=(s > 1 and start == 0), scale=self.scaling,
                                           enable_gqa=h != self.num_key_value_heads)
        return o.transpose(1, 2).reshape(b, s, h * d)

    def _forward_paged(self, xq: torch.Tensor, s1: torch.Tensor, cache: PagedKVCache, step: PagedStep) -> torch.Tensor:
        if not isinstance(step, PagedStep):
            raise RuntimeError("forward_int8: a PagedKVCache takes the PagedStep of cache.step(seq_ids, counts) in place of a start position")
        m = xq.shape[0]
        if xq.dim() != 2 or m != sum(step.counts):
            raise RuntimeError(f"forward_int8: xq must be [m, hidden] with the step's m = {sum(step.counts)} tokens packed in order")
        if not self._decode_supported():
            raise NotImplementedError(f"a paged KV cache needs head_dim 64 or 128, at most 8 query heads per KV head and h * head_dim <= "
                                      f"16384 (h={self.num_heads}, kvh={self.num_key_value_heads}, head_dim={self.head_dim})")
        # the tables grow in powers of two with the longest sequence, not with the pool (which may hold millions of keys)
        cos, sin = self.rope_tables(min(cache.capacity, max(1024, 1 << (step.max_len - 1).bit_length())))
        li = self.layer_idx
        lora = step.lora.layer(li) if step.lora is not None else None
        o_lora = lora("o_proj") if lora is not None else None
        q, k, v = self.project_qkv(xq, s1) if lora is None else self.project_qkv(xq, s1, lora)
        pools = (cache.k[li], cache.v[li]) + ((cache.k_scale[li], cache.v_scale[li]) if cache.quantized else ())
        if self.qk_norm:
            q_out = (ops.rope_qkv_norm_paged_kv8 if cache.quantized else ops.rope_qkv_norm_paged)(
                q, k, v, self.q_norm.weight, self.k_norm.weight, self.q_norm.eps, cos, sin, step.pos, step.slots, *pools)
        else:
            q_out = (ops.rope_qkv_paged_kv8 if cache.quantized else ops.rope_qkv_paged)(q, k, v, cos, sin, step.pos, step.slots, *pools)
        if step.decode and self._shared and step.family is not None:  # fuse_shared(): siblings read their common keys once per pack
            shared = ops.decode_attention_paged_shared_kv8 if cache.quantized else ops.decode_attention_paged_shared
            pack = min(int(step.family_max), 64 // (self.num_heads // self.num_key_value_heads))
            aq, a1 = shared(q_out, *pools, step.block_table, step.last_pos, step.family, step.shared, pack, self.scaling,
                            max_len=step.max_len)
            return forward_int8_lora(self.o_proj, aq, a1, o_lora)
        if step.decode:  # one token per sequence: the decode kernel through the block table, whatever fuse_decode() says
            decode = ops.decode_attention_paged_kv8 if cache.quantized else ops.decode_attention_paged
            aq, a1 = decode(q_out, *pools, step.block_table, step.last_pos, self.scaling, max_len=step.max_len)
            return forward_int8_lora(self.o_proj, aq, a1, o_lora)
        t = self._verify_tokens(step)
        if t:  # fuse_verify(): a uniform chunk of t tokens per sequence through the decode kernel's split over keys
            verify = ops.verify_attention_paged_kv8 if cache.quantized else ops.verify_attention_paged
            aq, a1 = verify(q_out, *pools, step.block_table, step.start_pos, t, self.scaling, max_len=step.max_len)
            return forward_int8_lora(self.o_proj, aq, a1, o_lora)
        if self._prefill:  # fuse_prefill(): the whole packed batch in one ragged causal attention over the pool, quantised for o_proj
            prefill = ops.prefill_attention_paged_kv8 if cache.quantized else ops.prefill_attention_paged
            aq, a1 = prefill(q_out, *pools, step.block_table, step.cu_tokens, step.start_pos, self.scaling, max_len=step.max_len)
            return forward_int8_lora(self.o_proj, aq, a1, o_lora)
        outs, t = [], 0
        for sid, c, start in zip(step.seq_ids, step.counts, step.starts):  # prefill / chunks: SDPA over a gathered copy, per sequence
            kc, vc = cache.gather(li, sid, start + c)
            outs.append(self._sdpa(q_out[t:t + c].transpose(0, 1)[None], kc, vc, start)[0])
            t += c
        aq, a1 = ops.dynamic_quant(torch.cat(outs) if len(outs) > 1 else outs[0])
        return forward_int8_lora(self.o_proj, aq.reshape(m, -1), a1.reshape(m, 1), o_lora)

    def forward_int8(self, xq: torch.Tensor, s1: torch.Tensor, cache: KVCache, start: int) -> torch.Tensor:
        if isinstance(cache, PagedKVCache):  # `start` is the PagedStep of this forward pass
            return self._forward_paged(xq, s1, cache, start)
        m = xq.shape[0]
        b = cache.batch
        if xq.dim() != 2 or m % b:
            raise RuntimeError(f"forward_int8: xq must be [batch * s, hidden] with batch = {b} (the cache's)")
        s = m // b
        if start < 0 or start + s > cache.capacity:
            raise RuntimeError(f"forward_int8: tokens {start} ... {start + s - 1} do not fit the cache capacity {cache.capacity}")
        if cache.quantized and not self._decode_supported():
            raise NotImplementedError(f"an int8 KV cache needs head_dim 64 or 128, at most 8 query heads per KV head and h * head_dim <= "
                                      f"16384 (h={self.num_heads}, kvh={self.num_key_value_heads}, head_dim={self.head_dim})")
        cos, sin = self.rope_tables(cache.capacity)
        q, k, v = self.project_qkv(xq, s1)
        pos = cache.positions(start, s)
        kc, vc = cache.k[self.layer_idx], cache.v[self.layer_idx]
        if cache.quantized:  # the int8 cache is the opt-in: one-token steps take its decode kernel whatever fuse_decode() says
            ksc, vsc = cache.k_scale[self.layer_idx], cache.v_scale[self.layer_idx]
            if self.qk_norm:
                q_out = ops.rope_qkv_norm_kv8(q, k, v, self.q_norm.weight, self.k_norm.weight, self.q_norm.eps, cos, sin, pos, kc, vc, ksc, vsc)
            else:
                q_out = ops.rope_qkv_kv8(q, k, v, cos, sin, pos, kc, vc, ksc, vsc)
            if s == 1:
                aq, a1 = ops.decode_attention_kv8(q_out, kc, vc, ksc, vsc, pos, self.scaling, max_len=start + 1)
                return self.o_proj.forward_int8(aq, a1)
        else:
            if self.qk_norm:
                q_out = ops.rope_qkv_norm(q, k, v, self.q_norm.weight, self.k_norm.weight, self.q_norm.eps, cos, sin, pos, kc, vc)
            else:
                q_out = ops.rope_qkv(q, k, v, cos, sin, pos, kc, vc)
            if self._decode and s == 1 and self._decode_supported():
                aq, a1 = ops.decode_attention(q_out, kc, vc, pos, self.scaling, max_len=start + 1)
                return self.o_proj.forward_int8(aq, a1)
        aq, a1 = ops.dynamic_quant(self.attend(q_out, cache, start))
        return self.o_proj.forward_int8(aq.reshape(m, -1), a1.reshape(m, 1))

    def forward(self, x: torch.Tensor, cache: KVCache, start: int) -> torch.Tensor:
        """x fp16 [b, s, hidden] or [b*s, hidden] -> the attention output of the same shape."""
        xq, s1 = ops.dynamic_quant(x.reshape(-1, x.shape[-1]).half())
        return self.forward_int8(xq, s1, cache, start).reshape(x.shape)


def _config_rope(config):
    """(rope_theta, rope dict or None) of a transformers config, 5.x (`rope_parameters`) or 4.x (`rope_theta`, `rope_scaling`) style."""
    rp = getattr(config, "rope_parameters", None)
    if isinstance(rp, dict) and rp:
        return float(rp.get("rope_theta", getattr(config, "rope_theta", 10000.0))), rp
    return float(getattr(config, "rope_theta", 10000.0)), getattr(config, "rope_scaling", None)


class QuantLlamaDecoderLayer(nn.Module):
    """Quantized{Llama,Qwen2}DecoderLayer: transformers' layer output
        h = hidden + self_attn(input_layernorm(hidden));  out = h + mlp(post_attention_layernorm(h))
    with every GEMM input produced already int8-quantised (QuantRMSNorm, silu_mul_quant) and the residual add of the second norm fused
    into it.  forward(hidden, cache, start): hidden fp16 [b, s, hidden] or [b*s, hidden], tokens at positions start ... start+s-1; with a
    PagedKVCache, forward(hidden, cache, step): hidden [m, hidden] packed as the PagedStep says."""

    def __init__(self, hidden: int, num_heads: int, num_kv_heads: int, intermediate: int, group_size: int, head_dim: Optional[int] = None,
                 qkv_bias: bool = False, o_bias: bool = False, rms_norm_eps: float = 1e-6, rope_theta: float = 10000.0,
                 rope_scaling: Optional[dict] = None, layer_idx: int = 0, qk_norm: bool = False):
        super().__init__()
        self.hidden_size = hidden
        self.self_attn = QuantLlamaAttention(hidden, num_heads, num_kv_heads, group_size, head_dim=head_dim, qkv_bias=qkv_bias,
                                             o_bias=o_bias, rope_theta=rope_theta, rope_scaling=rope_scaling, layer_idx=layer_idx,
                                             qk_norm=qk_norm, rms_norm_eps=rms_norm_eps)
        self.mlp = QuantLlamaMLP(hidden, intermediate, group_size)
        self.input_layernorm = QuantRMSNorm(hidden, eps=rms_norm_eps)
        self.post_attention_layernorm = QuantRMSNorm(hidden, eps=rms_norm_eps)

    @classmethod
    def from_config(cls, config, group_size: int, layer_idx: int = 0):
        """The layer of a transformers LlamaConfig, Qwen2Config or Qwen3Config (duck-typed, 4.x or 5.x attribute style).  Qwen2: q/k/v
        with bias, o without; Llama and Qwen3: all four follow `attention_bias`; Qwen3: q_norm / k_norm (qk_norm=True), head_dim from the
        config.  Sliding-window Qwen2 / Qwen3 (`use_sliding_window`, or a `layer_types` entry other than "full_attention") and rope types
        other than "default" / "llama3" raise NotImplementedError."""
        if getattr(config, "hidden_act", "silu") != "silu":
            raise NotImplementedError(f"hidden_act {config.hidden_act!r}: only SiLU MLPs are supported")
        qwen2 = getattr(config, "model_type", "") == "qwen2"
        qwen3 = getattr(config, "model_type", "") == "qwen3"
        if (qwen2 or qwen3) and getattr(config, "use_sliding_window", False):
            raise NotImplementedError("sliding-window attention is not supported")
        if qwen3 and any(t != "full_attention" for t in (getattr(config, "layer_types", None) or ())):
            raise NotImplementedError("layer_types other than 'full_attention' (sliding-window layers) are not supported")
        theta, rope = _config_rope(config)
        heads = config.num_attention_heads
        kv = getattr(config, "num_key_value_heads", None) or heads
        bias = bool(getattr(config, "attention_bias", False))
        return cls(config.hidden_size, heads, kv, config.intermediate_size, group_size,
                   head_dim=getattr(config, "head_dim", None) or config.hidden_size // heads,
                   qkv_bias=True if qwen2 else bias, o_bias=False if qwen2 else bias, rms_norm_eps=config.rms_norm_eps,
                   rope_theta=theta, rope_scaling=rope, layer_idx=layer_idx, qk_norm=qwen3)

    def fuse_decode(self):
        """self_attn.fuse_decode(): one-token steps take the split-K decode attention kernel.  Returns self."""
        self.self_attn.fuse_decode()
        return self

    def unfuse_decode(self):
        self.self_attn.unfuse_decode()
        return self

    @property
    def decode_fused(self) -> bool:
        return self.self_attn.decode_fused

    def fuse_prefill(self):
        """self_attn.fuse_prefill(): paged steps of more than one token take the paged prefill attention kernel.  Returns self."""
        self.self_attn.fuse_prefill()
        return self

    def unfuse_prefill(self):
        self.self_attn.unfuse_prefill()
        return self

    @property
    def prefill_fused(self) -> bool:
        return self.self_attn.prefill_fused

    def fuse_verify(self):
        """self_attn.fuse_verify(): uniform paged chunks of 2 ... 16 tokens per sequence take the verify attention kernel.  Returns self."""
        self.self_attn.fuse_verify()
        return self

    def unfuse_verify(self):
        self.self_attn.unfuse_verify()
        return self

    @property
    def verify_fused(self) -> bool:
        return self.self_attn.verify_fused

    def fuse_shared(self):
        """self_attn.fuse_shared(): paged decode steps over forked siblings take the shared-prefix decode attention kernel.  Returns self."""
        self.self_attn.fuse_shared()
        return self

    def unfuse_shared(self):
        self.self_attn.unfuse_shared()
        return self

    @property
    def shared_fused(self) -> bool:
        return self.self_attn.shared_fused

    def _lora(self, step):
        """the layer's adapters of a PagedStep that carries some (step.lora: a LoraStep), else None; a start position carries none"""
        held = getattr(step, "lora", None)
        return held.layer(self.self_attn.layer_idx) if held is not None else None

    def forward(self, hidden: torch.Tensor, cache: KVCache, start: int) -> torch.Tensor:
        x = hidden.reshape(-1, self.hidden_size)
        a = self.self_attn.forward_int8(*self.input_layernorm(x), cache, start)
        # a becomes h = fp16(a + x), torch's `residual + attn_out` (fp16 addition commutes), in the launch that quantises its norm
        mq, ms = self.post_attention_layernorm(x, a)
        return (a + forward_int8_lora(self.mlp, mq, ms, self._lora(start))).reshape(hidden.shape)

    def forward_chained(self, delta: torch.Tensor, residual: Optional[torch.Tensor], cache: KVCache, start: int):
        """The layer on a hidden state handed over as an unformed sum, hidden = residual + delta, returned the same way: (delta, residual)
        [tokens, hidden] -> (delta', residual') with forward(hidden) = fp16(residual' + delta').  The add that ends forward() is left to
        the next layer's input_layernorm (or the model's final norm), whose launch forms fp16(residual + delta) anyway: one launch per
        layer less, and bit for bit the chain of forward() calls, fp16 addition being correctly rounded and commutative.  `residual` is
        None for the first layer (delta is the hidden state itself) and is otherwise updated in place."""
        if residual is None:
            residual = delta.reshape(-1, self.hidden_size)
            xq, s1 = self.input_layernorm(residual)
        else:
            xq, s1 = self.input_layernorm(delta, residual)  # residual becomes the hidden state
        a = self.self_attn.forward_int8(xq, s1, cache, start)
        mq, ms = self.post_attention_layernorm(residual, a)  # a becomes h = hidden + attention
        return forward_int8_lora(self.mlp, mq, ms, self._lora(start)), a


__all__ = ["KVCache", "PagedKVCache", "PagedStep", "QuantLlamaAttention", "QuantLlamaDecoderLayer", "rope_inv_freq", "rope_tables"]
