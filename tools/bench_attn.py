#!/usr/bin/env python3
"""What the launches around the attention core cost per decoder layer: the transformers-style eager path against rope_qkv with the static
KV cache.  Both paths start from the fp16 output of input_layernorm and end with o_proj's output; every step is replayed from a hipGraph
(tools/bench_llama.time_fn).  Shapes: Llama-2-7B (hidden 4096, 32 / 32 heads of 128) and Llama-3-8B (32 / 8), per-channel and g128.

    unfused     q/k/v_proj.forward(y) (each quantises its own input); view + transpose; torch RoPE on q and k (apply_rotary_pos_emb with
                cos / sin gathered at the positions); DynamicCache-style torch.cat of the history and the new k / v; SDPA; transpose +
                contiguous; o_proj.forward
    fused       QuantLlamaAttention.forward(y): dynamic_quant once, q/k/v forward_int8, rope_qkv into the static cache, SDPA,
                dynamic_quant, o_proj.forward_int8
    fused_qkv   the same after fuse_qkv(): one q|k|v GEMM whose column ranges rope_qkv reads in place
    fused_decode  (decode points) fuse_qkv() + fuse_decode(): decode_attention (split-K over the cache, output int8-quantised) in place of
                SDPA and the dynamic_quant in front of o_proj
    fused_decode_kv8  (--kv8, decode points) the same with KVCache(dtype=torch.int8): rope_qkv_kv8 + decode_attention_kv8.  It is timed
                alternately with fused_decode, KV8_ROUNDS times each in the same process; both lists are kept (`*_runs`) and the medians
                reported (`fused_decode_alt`, `fused_decode_kv8`).  Prefill points get `fused_qkv_kv8` (SDPA over the dequantised cache).
    paged       (--paged [--block-size N], decode points) the same module over a PagedKVCache whose block tables are a random permutation of
                the pool: rope_qkv_paged + decode_attention_paged.  Contiguous (fused_decode) and paged are timed alternately, PAGED_ROUNDS
                times each in one process -- with --kv8 the two int8 paths join the rotation -- and every list is kept under `paged_runs`,
                the medians under `paged`.

    prefill_paged  (--points prefill --paged [--kv8] [--block-size N]: this mode alone) the module over a PagedKVCache at the packed steps of
                PAGED_PREFILL, with fuse_prefill() off -- per sequence PagedKVCache.gather, a mask, SDPA; then torch.cat and dynamic_quant:
                the baseline -- and on -- prefill_attention_paged, one ragged causal attention over the pool in place.  The off path builds
                index tensors on the host, so it cannot be captured: both are timed eagerly with events around each call, alternately,
                PREFILL_ROUNDS times in one process; every list is kept.  `faster` says whether the fused median is below the unfused one by
                more than the unfused path's spread over the rounds.  The attention op alone is timed from a hipGraph as well and its rate
                given against the nominal fp16 MFMA peak (FP16_PEAK_TFLOPS).

    verify      (--points verify [--kv8] [--block-size N]: this mode alone) the attention op of a speculative step's chunk alone, three ways
                over the same pool, block table and positions: verify_attention_paged(_kv8) for the chunk of T tokens per row,
                prefill_attention_paged(_kv8) for the same chunk (what the step ran before fuse_verify()), and decode_attention_paged(_kv8)
                for one token per row at the chunk's last position (the floor: the same keys once).  Each is replayed from a hipGraph
                (tools/bench_llama.time_fn), alternately, VERIFY_ROUNDS times in one process; every round is kept, with median, min and max.
                Shapes as above, b in {1, 16}, contexts {256, 4096, 16384} where the pool fits VERIFY_POOL_BYTES, T in {3, 5, 8}.
                `faster_than_prefill` says whether the verify median is below the prefill median by more than the latter's spread.

    shared      (--points shared [--kv8] [--block-size N]: this mode alone) the decode attention op of one family of N sibling rows alone,
                two ways over the same pool and the same forked block tables: decode_attention_paged_shared(_kv8) with pack = min(N,
                64 // (h / kvh)), and decode_attention_paged(_kv8) over the aliased tables (the baseline: every row reads the prefix's
                blocks for itself, from wherever the caches hold them).  Shapes as above, N in {2, 4, 8, 16}, prefixes of {1024, 4096,
                16384} shared keys and a private tail of SHARED_TAIL keys per row.  Two protocols, alternately, SHARED_ROUNDS times: `warm`
                (hipGraph replay back to back, tools/bench_llama.time_fn: the pools stay in whatever cache holds them) and `cold` (one
                captured call per timing, each behind a write of SHARED_FLUSH_BYTES that evicts the L2s and the Infinity Cache; median of
                SHARED_COLD_CALLS).  Every round is kept, with median, min and max; `shared_over_plain` per protocol, and `wins` / `loses`
                where the medians differ by more than the baseline's spread over the rounds.  The split plan of the call and the number of
                jointly taken splits are written too.

    qknorm      (--points qknorm [--block-size N]: this mode alone) the RoPE / cache-write launch of a Qwen3 layer alone, three ways over
                the same fused q|k|v buffer, positions, slots and pool: rope_qkv_norm_paged(_kv8) (`fused`: the per-head q / k RMSNorm
                inside the launch), the torch composition (`composed`: Qwen3RMSNorm's lines on the q and k views, then
                rope_qkv_paged(_kv8)), and rope_qkv_paged(_kv8) without any norm (`plain`: fused - plain is what the norm costs).  Qwen3-8B
                (32 / 8 heads of 128) and Qwen3-32B (64 / 8), {1, 16, 2048} tokens, fp16 and int8 pools.  The `cold` protocol of the shared
                points (one captured call per timing behind a cache flush, median of SHARED_COLD_CALLS), alternately, QKNORM_ROUNDS times;
                every round is kept, with median, min and max; `verdict` says wins / loses only where the medians differ by more than the
                composition's spread over the rounds.

Points: decode (s = 1) at b in {1, 16} with a context of {1024, 4096} tokens (the new token included), and b = 1 at 16384; prefill of s in
{128, 1024, 4096} tokens at b = 1 from position 0.  Before each point one dynamic_quant of POINT_MARK + i rows is launched: its grid marks
where point i starts in a kernel trace.

    python tools/bench_attn.py [--points decode,prefill] [--kv8] [--out FILE]   -> one JSON object on stdout
    python tools/bench_attn.py --points prefill --paged [--kv8] [--block-size N] [--out FILE]   -> the paged prefill points alone
    python tools/bench_attn.py --points verify [--kv8] [--block-size N] [--out profiles/verify_attn_bench.json]   -> the verify points alone
    python tools/bench_attn.py --points shared [--kv8] [--block-size N] [--out profiles/shared_attn_bench.json]   -> the shared points alone
    python tools/bench_attn.py --points qknorm [--block-size N] [--out profiles/qknorm_bench.json]   -> the q / k norm points alone
    python tools/bench_attn.py --summarize TRACE_DIR [--bench FILE]     -> from a rocprofv3 --kernel-trace run of the above: the
                                                                          qqq_rope_qkv_kernel times and HBM fractions, and per decode point
                                                                          (labelled from the run's JSON output FILE) the median times of
                                                                          the two decode-attention kernels, their K/V bytes as a fraction
                                                                          of 8 TB/s, and SDPA's attn_fwd; for a --paged run each split
                                                                          kernel's median per alternation and the paged kernels' excess
                                                                          over the contiguous ones against the latter's spread
"""
import argparse
import collections
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIDDEN, D = 4096, 128
SHAPES = {"llama2_7b": (32, 32), "llama3_8b": (32, 8)}
DECODE = [(b, ctx) for b in (1, 16) for ctx in (1024, 4096)] + [(1, 16384)]
POINT_MARK = 100000  # rows of the marker dynamic_quant launched before point i: POINT_MARK + i (no other call here has that many)
PREFILL = (128, 1024, 4096)
HBM_BYTES_PER_S = 8e12
ROPE_NT = 128  # qqq_w4a8.hip: ROPE_NT
KV8_ROUNDS = 3  # --kv8: alternations of fused_decode / fused_decode_kv8 at a decode point
PAGED_ROUNDS = 5  # --paged: alternations of the contiguous and the paged paths at a decode point
PREFILL_ROUNDS = 5  # --points prefill --paged: alternations of fuse_prefill() off and on at a point
PREFILL_CALLS = 7   # ... and event-timed calls per alternation (their median is the alternation's value)
FP16_PEAK_TFLOPS = 2500.0  # MI355X, dense fp16 MFMA (nominal)
# (name, [(start, count) per sequence]): a prompt, a batch of prompts, a late chunk, and that chunk batched with 15 decoding rows
PAGED_PREFILL = [("1x2048", [(0, 2048)]), ("8x512", [(0, 512)] * 8), ("chunk512@3584", [(3584, 512)]),
                 ("chunk512@3584+15dec@2048", [(3584, 512)] + [(2047, 1)] * 15)]
VERIFY_ROUNDS = 5  # --points verify: alternations of the three ops at a point
VERIFY_CONTEXTS, VERIFY_TOKENS, VERIFY_BATCHES = (256, 4096, 16384), (3, 5, 8), (1, 16)
VERIFY_POOL_BYTES = 8 << 30  # K and V pools of a point together
SHARED_ROUNDS, SHARED_COLD_CALLS = 5, 9  # --points shared: alternations of the two ops at a point; cold calls per alternation
SHARED_FAMILIES, SHARED_PREFIXES, SHARED_TAIL = (2, 4, 8, 16), (1024, 4096, 16384), 64
SHARED_FLUSH_BYTES = 1 << 30  # four times the 256 MB Infinity Cache
QKNORM_SHAPES = {"qwen3_8b": (32, 8), "qwen3_32b": (64, 8)}  # --points qknorm: (heads, KV heads) of 128
QKNORM_TOKENS, QKNORM_ROUNDS, QKNORM_EPS = (1, 16, 2048), 5, 1e-6
PREFILL_KERNELS = ("qqq_prefill_attn_kernel", "qqq_prefill_quant_kernel", "qqq_paged_rope_qkv_kernel", "qqq_paged_kv8_rope_qkv_kernel",
                   "qqq_dynamic_quant_kernel")
SPLIT_KERNELS = ("qqq_decode_split_kernel", "qqq_kv8_decode_split_kernel", "qqq_paged_decode_split_kernel",
                 "qqq_paged_kv8_decode_split_kernel")


def _rotate_half(x):
    import torch

    return torch.cat((-x[..., x.shape[-1] // 2:], x[..., : x.shape[-1] // 2]), dim=-1)


def _paged_decode_step(torch, dev, b, kvh, ctx, block_size, dtype):
    """(PagedKVCache, PagedStep): b sequences of ctx - 1 keys and the decode step that brings each to ctx, with the block ids replaced by
    a random permutation of the pool (the allocator hands blocks out in order; a serving pool after a while does not)"""
    import dataclasses

    from qqq_amd import PagedKVCache

    per = -(-ctx // block_size)
    cache = PagedKVCache(1, b * per, kvh, D, block_size, dev, dtype=dtype)
    for i in range(b):
        cache.add(i)
    if ctx > 1:
        cache.step(range(b), [ctx - 1] * b)
    step = cache.step(range(b), [1] * b)
    perm = torch.randperm(b * per, generator=torch.Generator().manual_seed(ctx + b)).to(dev)
    table = perm[step.block_table.long()].to(torch.int32)
    slots = perm[step.slots // block_size] * block_size + step.slots % block_size
    return cache, dataclasses.replace(step, block_table=table, slots=slots)


def run(points, group_sizes, kv8=False, paged=False, block_size=128):
    import torch
    import torch.nn.functional as F

    from bench_llama import make_ql, time_fn
    from qqq_amd import KVCache, QuantLlamaAttention, dynamic_quant

    dev = torch.device("cuda:0")
    out = {"hidden": HIDDEN, "head_dim": D, "unit": "us per call, hipGraph replay (median)", "points": []}
    if paged:
        out["block_size"] = block_size
    for shape, (h, kvh) in SHAPES.items():
        for gs in group_sizes:
            attn = QuantLlamaAttention(HIDDEN, h, kvh, gs).to(dev)
            attn.q_proj, attn.k_proj = make_ql(dev, h * D, HIDDEN, gs, 1), make_ql(dev, kvh * D, HIDDEN, gs, 2)
            attn.v_proj, attn.o_proj = make_ql(dev, kvh * D, HIDDEN, gs, 3), make_ql(dev, HIDDEN, h * D, gs, 4)
            runs = [("decode", b, ctx - 1, 1) for b, ctx in DECODE] if "decode" in points else []
            runs += [("prefill", 1, 0, s) for s in PREFILL] if "prefill" in points else []
            for kind, b, start, s in runs:
                cap = start + s
                cache = KVCache(1, b, kvh, D, cap, dev)
                cos, sin = attn.rope_tables(cap)
                y = (torch.randn((b * s, HIDDEN), device=dev) * 0.5).half()
                k_past = torch.randn((b, kvh, start, D), device=dev).half()
                v_past = torch.randn((b, kvh, start, D), device=dev).half()
                pos = torch.arange(start, start + s, device=dev)[None].expand(b, s)

                def unfused():
                    q = attn.q_proj.forward(y).view(b, s, h, D).transpose(1, 2)
                    k = attn.k_proj.forward(y).view(b, s, kvh, D).transpose(1, 2)
                    v = attn.v_proj.forward(y).view(b, s, kvh, D).transpose(1, 2)
                    c, sn = cos[pos].unsqueeze(1), sin[pos].unsqueeze(1)
                    q = (q * c) + (_rotate_half(q) * sn)
                    k = (k * c) + (_rotate_half(k) * sn)
                    kk, vv = torch.cat((k_past, k), dim=-2), torch.cat((v_past, v), dim=-2)
                    o = F.scaled_dot_product_attention(q, kk, vv, is_causal=s > 1, scale=D ** -0.5, enable_gqa=h != kvh)
                    return attn.o_proj.forward(o.transpose(1, 2).contiguous().reshape(b * s, h * D))

                def fused():
                    return attn.forward(y, cache, start)

                dynamic_quant(torch.zeros((POINT_MARK + len(out["points"]), 8), dtype=torch.float16, device=dev))
                pt = {"shape": shape, "heads": h, "kv_heads": kvh, "group_size": gs, "kind": kind, "batch": b, "tokens": s,
                      "context": start + s}
                attn.unfuse_qkv()
                pt["unfused"] = round(time_fn(unfused), 2)
                pt["fused"] = round(time_fn(fused), 2)
                attn.fuse_qkv()
                pt["fused_qkv"] = round(time_fn(fused), 2)
                if kind == "decode":
                    attn.fuse_decode()
                    pt["fused_decode"] = round(time_fn(fused), 2)
                    attn.unfuse_decode()
                if kv8:
                    cache8 = KVCache(1, b, kvh, D, cap, dev, dtype=torch.int8)

                    def fused8():
                        return attn.forward(y, cache8, start)

                    if kind == "decode":
                        attn.fuse_decode()
                        alt, alt8 = [], []
                        for _ in range(KV8_ROUNDS):
                            alt.append(round(time_fn(fused), 2))
                            alt8.append(round(time_fn(fused8), 2))
                        attn.unfuse_decode()
                        pt.update({"fused_decode_alt": _median(alt), "fused_decode_kv8": _median(alt8), "fused_decode_alt_runs": alt,
                                   "fused_decode_kv8_runs": alt8})
                    else:
                        pt["fused_qkv_kv8"] = round(time_fn(fused8), 2)
                    del cache8
                if paged and kind == "decode":
                    # contiguous and paged module paths in rotation, fuse_qkv() and fuse_decode() on: name -> (cache, start or PagedStep)
                    variants = {"fused_decode": (cache, start), "paged": _paged_decode_step(torch, dev, b, kvh, cap, block_size, torch.float16)}
                    if kv8:
                        variants["fused_decode_kv8"] = (KVCache(1, b, kvh, D, cap, dev, dtype=torch.int8), start)
                        variants["paged_kv8"] = _paged_decode_step(torch, dev, b, kvh, cap, block_size, torch.int8)
                    attn.fuse_decode()
                    lists = {name: [] for name in variants}
                    for _ in range(PAGED_ROUNDS):
                        for name, (c_, st_) in variants.items():
                            lists[name].append(round(time_fn(lambda: attn.forward(y, c_, st_)), 2))
                    attn.unfuse_decode()
                    pt["paged"] = {name: _median(v) for name, v in lists.items()}
                    pt["paged_runs"] = lists
                    del variants
                attn.unfuse_qkv()
                pt["saved"] = round(pt["unfused"] - pt["fused"], 2)
                pt["saved_qkv"] = round(pt["unfused"] - pt["fused_qkv"], 2)
                out["points"].append(pt)
                print(json.dumps(pt), file=sys.stderr, flush=True)
                del cache, k_past, v_past
                torch.cuda.empty_cache()
    return out


def _median(v):
    v = sorted(v)
    return round(v[len(v) // 2], 2)


def _paged_prefill_step(torch, dev, seqs, kvh, block_size, dtype):
    """(PagedKVCache, PagedStep) of a packed step of (start, count) sequences whose histories are in the pool; the allocator's free list is
    shuffled first, so block tables, slots and gather() all see a random permutation of the pool"""
    import random

    from qqq_amd import PagedKVCache

    nb = sum(-(-(s + c) // block_size) for s, c in seqs)
    cache = PagedKVCache(1, nb, kvh, D, block_size, dev, dtype=dtype)
    random.Random(nb).shuffle(cache._free)
    for i, (s, _) in enumerate(seqs):
        cache.add(i)
        if s:
            cache.step([i], [s])
    g = torch.Generator(device=dev).manual_seed(nb)
    for t in cache.k + cache.v:  # a history: random rows (random codes and scales for an int8 pool)
        if dtype == torch.int8:
            t.copy_(torch.randint(-127, 128, t.shape, generator=g, device=dev, dtype=torch.int8))
        else:
            t.copy_(torch.randn(t.shape, generator=g, device=dev).half())
    if dtype == torch.int8:
        for t in cache.k_scale + cache.v_scale:
            t.copy_(torch.rand(t.shape, generator=g, device=dev) * 0.02 + 0.005)
    return cache, cache.step(range(len(seqs)), [c for _, c in seqs])


def _time_eager(torch, fn, calls):
    """median GPU time of one eager call in us, events around each call (launch gaps of the call included, as a serving loop sees them)"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    v = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        v.append(a.elapsed_time(b) * 1e3)
    return _median(v)


def run_paged_prefill(group_sizes, kv8=False, block_size=128):
    import torch

    from bench_llama import make_ql, time_fn
    from qqq_amd import QuantLlamaAttention, dynamic_quant, ops

    dev = torch.device("cuda:0")
    out = {"hidden": HIDDEN, "head_dim": D, "block_size": block_size, "rounds": PREFILL_ROUNDS, "calls_per_round": PREFILL_CALLS,
           "unit": "us per module call (fp16 norm output -> o_proj output), eager, events around each call; median of the rounds' medians",
           "fp16_peak_tflops_nominal": FP16_PEAK_TFLOPS, "points": []}
    for shape, (h, kvh) in SHAPES.items():
        for gs in group_sizes:
            attn = QuantLlamaAttention(HIDDEN, h, kvh, gs).to(dev)
            attn.q_proj, attn.k_proj = make_ql(dev, h * D, HIDDEN, gs, 1), make_ql(dev, kvh * D, HIDDEN, gs, 2)
            attn.v_proj, attn.o_proj = make_ql(dev, kvh * D, HIDDEN, gs, 3), make_ql(dev, HIDDEN, h * D, gs, 4)
            attn.fuse_qkv()
            for name, seqs in PAGED_PREFILL:
                for dtype in (torch.float16,) + ((torch.int8,) if kv8 else ()):
                    cache, step = _paged_prefill_step(torch, dev, seqs, kvh, block_size, dtype)
                    m = sum(step.counts)
                    y = (torch.randn((m, HIDDEN), device=dev) * 0.5).half()
                    dynamic_quant(torch.zeros((POINT_MARK + len(out["points"]), 8), dtype=torch.float16, device=dev))
                    lists = {"unfused": [], "fused": []}
                    for _ in range(PREFILL_ROUNDS):
                        attn.unfuse_prefill()
                        lists["unfused"].append(_time_eager(torch, lambda: attn.forward(y, cache, step), PREFILL_CALLS))
                        attn.fuse_prefill()
                        lists["fused"].append(_time_eager(torch, lambda: attn.forward(y, cache, step), PREFILL_CALLS))
                    attn.unfuse_prefill()
                    # the attention op alone, from a hipGraph: its launches are shape-only
                    q_out = torch.randn((m, h, D), device=dev).half()
                    pools = (cache.k[0], cache.v[0]) + ((cache.k_scale[0], cache.v_scale[0]) if cache.quantized else ())
                    op = ops.prefill_attention_paged_kv8 if cache.quantized else ops.prefill_attention_paged
                    op_us = time_fn(lambda: op(q_out, *pools, step.block_table, step.cu_tokens, step.start_pos, D ** -0.5,
                                               max_len=step.max_len))
                    flops = sum(4 * D * h * (2 * s + c + 1) * c // 2 for s, c in seqs)  # 2 * 2 d per (token, head, attended key)
                    mu, mf = _median(lists["unfused"]), _median(lists["fused"])
                    spread = round(max(lists["unfused"]) - min(lists["unfused"]), 2)
                    pt = {"shape": shape, "heads": h, "kv_heads": kvh, "group_size": gs, "kind": "prefill_paged", "step": name,
                          "kv_dtype": "int8" if cache.quantized else "fp16", "tokens": m, "sequences": len(seqs), "unfused": mu, "fused": mf,
                          "unfused_spread": spread, "ratio": round(mu / mf, 3), "faster": bool(mu - mf > spread),
                          "gated": "dec@" not in name, "runs": lists, "attention_op_us": round(op_us, 2), "attention_flops": flops,
                          "attention_tflops": round(flops / op_us * 1e-6, 1),
                          "fraction_of_fp16_peak": round(flops / op_us * 1e-6 / FP16_PEAK_TFLOPS, 4)}
                    out["points"].append(pt)
                    print(json.dumps(pt), file=sys.stderr, flush=True)
                    del cache, step, pools
                    torch.cuda.empty_cache()
    return out


def summarize_prefill(trace_dir, bench=None):
    """kernel medians of a rocprofv3 --kernel-trace run of --points prefill --paged, per point (between the marker launches)"""
    from code_object import _demangle

    rows_all = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows_all += list(csv.DictReader(open(f)))
    per_point = collections.defaultdict(lambda: collections.defaultdict(list))
    point = None
    for r in sorted(rows_all, key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"]
        name = name[5:] if name.startswith("void ") else name
        name = name.split("(")[0]
        name = _demangle(name) if name.startswith("_Z") else name
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        grid = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
        if name.startswith("qqq_dynamic_quant_kernel") and grid >= POINT_MARK:
            point = grid - POINT_MARK
            continue
        if point is None:
            continue
        key = next((k for k in PREFILL_KERNELS if name.startswith(k)), "attn_fwd" if "attn_fwd" in name or "fmha" in name.lower() else None)
        if key:
            per_point[point][key].append(us)
    points = json.load(open(bench))["points"] if bench else []
    rows = []
    for i, ks in sorted(per_point.items()):
        pt = points[i] if i < len(points) else {}
        row = {"point": i}
        row.update({k: pt[k] for k in ("shape", "group_size", "step", "kv_dtype", "tokens", "attention_flops") if k in pt})
        for key, v in ks.items():
            row[key + "_median_us"], row[key + "_calls"] = _median(v), len(v)
        if "qqq_prefill_attn_kernel" in ks and "attention_flops" in pt:
            tf = pt["attention_flops"] / row["qqq_prefill_attn_kernel_median_us"] * 1e-6
            row.update({"prefill_attn_kernel_tflops": round(tf, 1), "fraction_of_fp16_peak": round(tf / FP16_PEAK_TFLOPS, 4)})
        rows.append(row)
    return {"unit": "kernel time from rocprofv3 --kernel-trace (median over calls), us", "fp16_peak_tflops_nominal": FP16_PEAK_TFLOPS,
            "points": rows}


def summarize(trace_dir, bench=None):
    from code_object import _demangle

    times = collections.defaultdict(list)
    per_point = collections.defaultdict(lambda: collections.defaultdict(list))  # point -> kernel -> [us]
    rows_all = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows_all += list(csv.DictReader(open(f)))
    point = None
    alternations = collections.defaultdict(lambda: collections.defaultdict(list))  # point -> split kernel -> [[us] per alternation]
    last_split = {}
    for r in sorted(rows_all, key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"]
        name = name[5:] if name.startswith("void ") else name
        name = name.split("(")[0]
        name = _demangle(name) if name.startswith("_Z") else name
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        grid = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
        if name.startswith("qqq_dynamic_quant_kernel") and grid >= POINT_MARK:
            point = grid - POINT_MARK
            continue
        if point is not None:
            for key in SPLIT_KERNELS + ("qqq_decode_combine_kernel", "attn_fwd"):
                if name.startswith(key) or (key == "attn_fwd" and "attn_fwd" in name):
                    per_point[point][key].append(us)
                    if key in SPLIT_KERNELS:  # an alternation: a run of launches of one split kernel that another one ends
                        if last_split.get(point) != key:
                            alternations[point][key].append([])
                            last_split[point] = key
                        alternations[point][key][-1].append(us)
        if name.startswith("qqq_rope_qkv_kernel"):
            gy = int(r.get("Grid_Size_Y", 1)) // max(1, int(r.get("Workgroup_Size_Y", 1)))
            times[(grid, gy)].append(us)
    # the shape behind a launch: grid y = ceil((h + 2 kvh) * D / 16 / ROPE_NT) blocks
    by_gy = {-(-(h + 2 * kvh) * (D // 16) // ROPE_NT): (name, h, kvh) for name, (h, kvh) in SHAPES.items()}
    rows = []
    for (m, gy), v in sorted(times.items()):
        if gy not in by_gy:
            continue
        name, h, kvh = by_gy[gy]
        v = sorted(v)
        med = v[len(v) // 2]
        width = (h + 2 * kvh) * D
        nbytes = m * width * 2 * 2 + m * D * 2 * 2  # q|k|v read + q, k, v written; one cos and one sin row per token
        rows.append({"kernel": "qqq_rope_qkv_kernel", "shape": name, "tokens": m, "calls": len(v), "median_us": round(med, 2),
                     "min_us": round(v[0], 2), "bytes": nbytes, "hbm_fraction_of_8TBps": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 4)})
    points = json.load(open(bench))["points"] if bench else []
    decode = []
    for i, ks in sorted(per_point.items()):
        pt = points[i] if i < len(points) else {}
        row = {"point": i}
        row.update({k: pt[k] for k in ("shape", "group_size", "kind", "batch", "context", "fused_qkv", "fused_decode", "fused_decode_alt",
                                       "fused_decode_kv8", "paged") if k in pt})
        for key, v in ks.items():
            row[key + "_median_us"], row[key + "_calls"] = _median(v), len(v)
        if "qqq_decode_split_kernel" in ks and "context" in pt:
            both = row["qqq_decode_split_kernel_median_us"] + row.get("qqq_decode_combine_kernel_median_us", 0.0)
            kv = 2 * pt["batch"] * pt["kv_heads"] * pt["context"] * D * 2  # K and V, fp16
            row.update({"decode_kernels_us": round(both, 2), "kv_bytes": kv, "kv_fraction_of_8TBps": round(kv / (both * 1e-6) / HBM_BYTES_PER_S, 4)})
        if "qqq_kv8_decode_split_kernel" in ks and "context" in pt:
            # the int8 cache: d codes and one f32 scale per (token, KV head), K and V; the combine kernel's calls are both modes' together
            both = row["qqq_kv8_decode_split_kernel_median_us"] + row.get("qqq_decode_combine_kernel_median_us", 0.0)
            kv = 2 * pt["batch"] * pt["kv_heads"] * pt["context"] * (D + 4)
            row.update({"kv8_decode_kernels_us": round(both, 2), "kv8_bytes": kv,
                        "kv8_fraction_of_8TBps": round(kv / (both * 1e-6) / HBM_BYTES_PER_S, 4)})
            for key in ("qqq_decode_split_kernel", "qqq_kv8_decode_split_kernel"):  # the spread the two medians are compared against
                v = sorted(ks.get(key, []))
                if v:
                    row[key + "_p10_us"], row[key + "_p90_us"] = round(v[len(v) // 10], 2), round(v[(9 * len(v)) // 10], 2)
        # a --paged run: the paged split kernel against the contiguous one of the same point.  The yardstick is the contiguous kernel's own
        # run-to-run spread: the range of its per-alternation medians
        for cont, pg in (("qqq_decode_split_kernel", "qqq_paged_decode_split_kernel"),
                         ("qqq_kv8_decode_split_kernel", "qqq_paged_kv8_decode_split_kernel")):
            if cont in ks and pg in ks:
                meds = {k: [_median(a) for a in alternations[i][k]] for k in (cont, pg)}
                spread = round(max(meds[cont]) - min(meds[cont]), 2)
                excess = round(_median(ks[pg]) - _median(ks[cont]), 2)
                row[pg + "_vs_contiguous"] = {"contiguous_median_us": _median(ks[cont]), "paged_median_us": _median(ks[pg]),
                                              "excess_us": excess, "contiguous_spread_us": spread, "within_spread": excess <= spread,
                                              "contiguous_alternation_medians_us": meds[cont], "paged_alternation_medians_us": meds[pg]}
        decode.append(row)
    return {"unit": "kernel time from rocprofv3 --kernel-trace (median over calls)", "kernels": rows, "points": decode}


def run_verify(kv8=False, block_size=128):
    """--points verify: see the module docstring; --kv8 adds the int8 pool's points behind the fp16 pool's"""
    out = _run_verify(False, block_size)
    if kv8:
        more = _run_verify(True, block_size)
        out["pool"] = "fp16, then int8"
        out["points"] += more["points"]
        out["skipped"] += more["skipped"]
    return out


def _run_verify(kv8, block_size):
    import statistics

    import torch

    from bench_llama import time_fn
    from qqq_amd import ops

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_attn.py --points verify", "device": torch.cuda.get_device_name(0),
           "head_dim": D, "block_size": block_size, "pool": "int8" if kv8 else "fp16", "rounds": VERIFY_ROUNDS,
           "unit": "us per call of the attention op alone, hipGraph replay (median of a round's replays); per op the rounds, their median, "
                   "min and max", "points": [], "skipped": []}
    g = torch.Generator(device=dev).manual_seed(7)
    for shape, (h, kvh) in SHAPES.items():
        for b in VERIFY_BATCHES:
            for ctx in VERIFY_CONTEXTS:  # keys a row holds once the chunk is written: the last token sits at ctx - 1
                per = -(-ctx // block_size)
                nb = b * per
                nbytes = 2 * nb * kvh * block_size * (D + 4 if kv8 else 2 * D)
                if nbytes > VERIFY_POOL_BYTES:
                    out["skipped"].append({"shape": shape, "pool": "int8" if kv8 else "fp16", "batch": b, "context": ctx, "why": f"pools of {nbytes >> 20} MiB"})
                    continue
                if kv8:
                    pools = tuple(torch.randint(-127, 128, (nb, kvh, block_size, D), generator=g, device=dev, dtype=torch.int8)
                                  for _ in range(2))
                    pools += tuple(torch.rand((nb, kvh, block_size), generator=g, device=dev) * 0.02 + 0.005 for _ in range(2))
                else:
                    pools = tuple(torch.randn((nb, kvh, block_size, D), generator=g, device=dev).half() for _ in range(2))
                table = torch.randperm(nb, generator=torch.Generator().manual_seed(ctx + b)).to(dev).reshape(b, per).to(torch.int32)
                last = torch.full((b,), ctx - 1, dtype=torch.int64, device=dev)
                q1 = torch.randn((b, h, D), generator=g, device=dev).half()
                decode = ops.decode_attention_paged_kv8 if kv8 else ops.decode_attention_paged
                verify = ops.verify_attention_paged_kv8 if kv8 else ops.verify_attention_paged
                prefill = ops.prefill_attention_paged_kv8 if kv8 else ops.prefill_attention_paged
                for t in VERIFY_TOKENS:
                    start = last - (t - 1)
                    cu = torch.arange(b + 1, dtype=torch.int32, device=dev) * t
                    q = torch.randn((b * t, h, D), generator=g, device=dev).half()
                    fns = {"verify": lambda: verify(q, *pools, table, start, t, D ** -0.5, max_len=ctx),
                           "prefill": lambda: prefill(q, *pools, table, cu, start, D ** -0.5, max_len=ctx),
                           "decode": lambda: decode(q1, *pools, table, last, D ** -0.5, max_len=ctx)}
                    runs = {name: [] for name in fns}
                    for _ in range(VERIFY_ROUNDS):
                        for name, fn in fns.items():
                            runs[name].append(round(time_fn(fn), 2))
                    pt = {"shape": shape, "pool": "int8" if kv8 else "fp16", "heads": h, "kv_heads": kvh, "batch": b, "context": ctx, "tokens": t}
                    for name, v in runs.items():
                        pt[name] = {"median_us": round(statistics.median(v), 2), "min_us": min(v), "max_us": max(v), "rounds_us": v}
                    spread = round(pt["prefill"]["max_us"] - pt["prefill"]["min_us"], 2)
                    pt["verify_over_prefill"] = round(pt["verify"]["median_us"] / pt["prefill"]["median_us"], 3)
                    pt["verify_over_decode"] = round(pt["verify"]["median_us"] / pt["decode"]["median_us"], 3)
                    pt["prefill_round_spread_us"] = spread
                    pt["faster_than_prefill"] = bool(pt["verify"]["median_us"] < pt["prefill"]["median_us"] - spread)
                    out["points"].append(pt)
                    print(json.dumps(pt), file=sys.stderr, flush=True)
                del pools
    return out


def run_shared(kv8=False, block_size=128):
    """--points shared: see the module docstring; --kv8 adds the int8 pool's points behind the fp16 pool's"""
    out = _run_shared(False, block_size)
    if kv8:
        out["pool"] = "fp16, then int8"
        out["points"] += _run_shared(True, block_size)["points"]
    return out


def _time_cold(torch, fn, flush, calls):
    """median us of single captured calls of fn, each behind a write that evicts the caches"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        flush.add_(1)
        a.record()
        graph.replay()
        b.record()
    torch.cuda.synchronize()
    return _median([a.elapsed_time(b) * 1e3 for a, b in ev])


def _run_shared(kv8, block_size):
    import statistics

    import torch

    from bench_llama import time_fn
    from qqq_amd import ops

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_attn.py --points shared", "device": torch.cuda.get_device_name(0), "head_dim": D, "block_size": block_size,
           "pool": "int8" if kv8 else "fp16", "rounds": SHARED_ROUNDS, "private_tail_keys": SHARED_TAIL,
           "unit": "us per call of the attention op alone; warm: hipGraph replay back to back; cold: one captured call behind a cache "
                   "flush, median of %d; per op and protocol the rounds, their median, min and max" % SHARED_COLD_CALLS, "points": []}
    g = torch.Generator(device=dev).manual_seed(11)
    flush = torch.zeros(SHARED_FLUSH_BYTES // 4, dtype=torch.int32, device=dev)
    plain = ops.decode_attention_paged_kv8 if kv8 else ops.decode_attention_paged
    joint = ops.decode_attention_paged_shared_kv8 if kv8 else ops.decode_attention_paged_shared
    for shape, (h, kvh) in SHAPES.items():
        for prefix in SHARED_PREFIXES:
            for n in SHARED_FAMILIES:
                ctx = prefix + SHARED_TAIL  # keys of a row, its newest included
                width, common = -(-ctx // block_size), prefix // block_size
                nb = common + n * (width - common)
                if kv8:
                    pools = tuple(torch.randint(-127, 128, (nb, kvh, block_size, D), generator=g, device=dev, dtype=torch.int8)
                                  for _ in range(2))
                    pools += tuple(torch.rand((nb, kvh, block_size), generator=g, device=dev) * 0.02 + 0.005 for _ in range(2))
                else:
                    pools = tuple(torch.randn((nb, kvh, block_size, D), generator=g, device=dev).half() for _ in range(2))
                perm = torch.randperm(nb, generator=torch.Generator().manual_seed(prefix + n))
                table = torch.empty((n, width), dtype=torch.int32)
                table[:, :common] = perm[:common]
                table[:, common:] = perm[common:].reshape(n, width - common)
                table = table.to(dev)
                pos = torch.full((n,), ctx - 1, dtype=torch.int64, device=dev)
                family = torch.zeros(n, dtype=torch.int32, device=dev)
                shared = torch.full((n,), common * block_size, dtype=torch.int64, device=dev)
                pack = min(n, 64 // (h // kvh))
                q = torch.randn((n, h, D), generator=g, device=dev).half()
                fns = {"plain": lambda: plain(q, *pools, table, pos, D ** -0.5, max_len=ctx),
                       "shared": lambda: joint(q, *pools, table, pos, family, shared, pack, D ** -0.5, max_len=ctx)}
                a, b_ = fns["plain"](), fns["shared"]()
                assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1]), "the two ops must agree bit for bit"
                splits, chunk = ops.decode_attention_shared_plan(n, h, kvh, ctx, pack)
                runs = {(name, mode): [] for name in fns for mode in ("warm", "cold")}
                for _ in range(SHARED_ROUNDS):
                    for name, fn in fns.items():
                        runs[(name, "warm")].append(round(time_fn(fn), 2))
                        runs[(name, "cold")].append(round(_time_cold(torch, fn, flush, SHARED_COLD_CALLS), 2))
                pt = {"shape": shape, "pool": "int8" if kv8 else "fp16", "heads": h, "kv_heads": kvh, "family": n, "pack": pack,
                      "prefix": prefix, "context": ctx, "splits": splits, "chunk": chunk, "joint_splits": common * block_size // chunk}
                for mode in ("warm", "cold"):
                    for name in fns:
                        v = runs[(name, mode)]
                        pt[f"{name}_{mode}"] = {"median_us": round(statistics.median(v), 2), "min_us": min(v), "max_us": max(v), "rounds_us": v}
                    base, new = pt[f"plain_{mode}"], pt[f"shared_{mode}"]
                    spread = round(base["max_us"] - base["min_us"], 2)
                    pt[f"shared_over_plain_{mode}"] = round(new["median_us"] / base["median_us"], 3)
                    pt[f"plain_round_spread_us_{mode}"] = spread
                    pt[f"verdict_{mode}"] = ("wins" if new["median_us"] < base["median_us"] - spread else
                                             "loses" if new["median_us"] > base["median_us"] + spread else "ties")
                out["points"].append(pt)
                print(json.dumps(pt), file=sys.stderr, flush=True)
                del pools
    return out


def run_qknorm(block_size=128):
    """--points qknorm: see the module docstring"""
    import statistics

    import torch

    from qqq_amd import ops

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_attn.py --points qknorm", "device": torch.cuda.get_device_name(0), "head_dim": D, "block_size": block_size,
           "eps": QKNORM_EPS, "rounds": QKNORM_ROUNDS,
           "unit": "us per call; cold: one captured call behind a cache flush, median of %d; per op the rounds, their median, min and max"
                   % SHARED_COLD_CALLS, "points": []}
    g = torch.Generator(device=dev).manual_seed(13)
    flush = torch.zeros(SHARED_FLUSH_BYTES // 4, dtype=torch.int32, device=dev)

    def hf_norm(x, w):  # transformers' Qwen3RMSNorm.forward, line for line
        dtype = x.dtype
        x = x.to(torch.float32)
        variance = x.pow(2).mean(-1, keepdim=True)
        x = x * torch.rsqrt(variance + QKNORM_EPS)
        return w * x.to(dtype)

    for shape, (h, kvh) in QKNORM_SHAPES.items():
        for kv8 in (False, True):
            for m in QKNORM_TOKENS:
                nb = -(-m // block_size) + 1
                if kv8:
                    pools = tuple(torch.zeros((nb, kvh, block_size, D), dtype=torch.int8, device=dev) for _ in range(2))
                    pools += tuple(torch.zeros((nb, kvh, block_size), dtype=torch.float32, device=dev) for _ in range(2))
                else:
                    pools = tuple(torch.zeros((nb, kvh, block_size, D), dtype=torch.float16, device=dev) for _ in range(2))
                nq, nk = h * D, kvh * D
                qkv = torch.randn((m, nq + 2 * nk), generator=g, device=dev).half()  # the fused GEMM's output, read in place
                q, k, v = qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:]
                qw = (1 + 0.3 * torch.randn(D, generator=g, device=dev)).half()
                kw = (1 + 0.3 * torch.randn(D, generator=g, device=dev)).half()
                cos, sin = (torch.rand((m + 8, D), generator=g, device=dev) * 2 - 1).half(), (torch.rand((m + 8, D), generator=g, device=dev) * 2 - 1).half()
                pos = torch.arange(m, device=dev)
                slots = torch.randperm(nb * block_size, generator=torch.Generator().manual_seed(m))[:m].to(dev)
                fused_op = ops.rope_qkv_norm_paged_kv8 if kv8 else ops.rope_qkv_norm_paged
                plain_op = ops.rope_qkv_paged_kv8 if kv8 else ops.rope_qkv_paged
                fns = {"fused": lambda: fused_op(q, k, v, qw, kw, QKNORM_EPS, cos, sin, pos, slots, *pools),
                       "composed": lambda: plain_op(hf_norm(q.view(m, h, D), qw).view(m, nq), hf_norm(k.view(m, kvh, D), kw).view(m, nk), v,
                                                    cos, sin, pos, slots, *pools),
                       "plain": lambda: plain_op(q, k, v, cos, sin, pos, slots, *pools)}
                runs = {name: [] for name in fns}
                for _ in range(QKNORM_ROUNDS):
                    for name, fn in fns.items():
                        runs[name].append(round(_time_cold(torch, fn, flush, SHARED_COLD_CALLS), 2))
                pt = {"shape": shape, "pool": "int8" if kv8 else "fp16", "heads": h, "kv_heads": kvh, "tokens": m}
                for name, r in runs.items():
                    pt[name] = {"median_us": round(statistics.median(r), 2), "min_us": min(r), "max_us": max(r), "rounds_us": r}
                spread = round(pt["composed"]["max_us"] - pt["composed"]["min_us"], 2)
                pt["composed_round_spread_us"] = spread
                pt["fused_over_composed"] = round(pt["fused"]["median_us"] / pt["composed"]["median_us"], 3)
                pt["norm_cost_us"] = round(pt["fused"]["median_us"] - pt["plain"]["median_us"], 2)  # what the norm adds to the launch
                pt["plain_round_spread_us"] = round(pt["plain"]["max_us"] - pt["plain"]["min_us"], 2)
                pt["verdict"] = ("wins" if pt["fused"]["median_us"] < pt["composed"]["median_us"] - spread else
                                 "loses" if pt["fused"]["median_us"] > pt["composed"]["median_us"] + spread else "ties")
                out["points"].append(pt)
                print(json.dumps(pt), file=sys.stderr, flush=True)
                del pools
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="decode,prefill")
    ap.add_argument("--group-sizes", default="-1,128")
    ap.add_argument("--kv8", action="store_true", help="also time the int8 KV cache (fused_decode_kv8 / fused_qkv_kv8)")
    ap.add_argument("--paged", action="store_true", help="decode points: time the contiguous and the paged module path alternately; "
                    "with --points prefill alone: the paged prefill points, fuse_prefill() off against on")
    ap.add_argument("--block-size", type=int, default=128, help="--paged: keys per block (a power of two in [16, 256])")
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarize", default=None, metavar="TRACE_DIR")
    ap.add_argument("--bench", default=None, metavar="FILE", help="--summarize: the JSON output of the traced run, to label the points")
    a = ap.parse_args()
    if a.summarize:
        res = summarize_prefill(a.summarize, a.bench) if a.paged and a.points == "prefill" else summarize(a.summarize, a.bench)
    elif a.points == "verify":
        res = run_verify(kv8=a.kv8, block_size=a.block_size)
    elif a.points == "shared":
        res = run_shared(kv8=a.kv8, block_size=a.block_size)
    elif a.points == "qknorm":
        res = run_qknorm(block_size=a.block_size)
    elif a.paged and a.points == "prefill":
        res = run_paged_prefill([int(v) for v in a.group_sizes.split(",")], kv8=a.kv8, block_size=a.block_size)
    else:
        res = run(a.points.split(","), [int(v) for v in a.group_sizes.split(",")], kv8=a.kv8, paged=a.paged, block_size=a.block_size)
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
