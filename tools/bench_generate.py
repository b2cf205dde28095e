#!/usr/bin/env python3
"""Generation end to end, decode time per token, three ways in one process: a Llama-2-7B-shaped model of four layers (hidden 4096, 32 heads
of 128, intermediate 11008, vocab 32000, per-channel W4A8, fuse_qkv()) over a paged fp16 cache, prompts of 128 tokens, 128 new tokens, greedy.

    generate        QuantLlamaForCausalLM.generate(device_loop=False): a host-built step, eager launches and a tolist() per token
    loop eager      DecodeLoop(graph=False): the step's metadata on the device, eager launches, a host sync every `sync_every` tokens
    loop graph      DecodeLoop(graph=True): the same, the step replayed from one captured graph

A round times every variant once, alternately.  A variant's value in a round is (wall time of a run with NEW tokens - wall time of a run with
1 token) / (NEW - 1): the prefill and the first token are in both runs, the NEW - 1 decode steps in one.  Both runs end in a device
synchronise.  The wall time of the 1-token run -- admission, the prefill and the first token -- is written beside it (one_token_us).  The
capture happens in the warm-up, outside the timed runs.  Written: the per-round values, their median, min and max, the ratio generate /
loop graph, and at batch 1 whether the captured loop's median lies below generate's by more than generate's own round-to-round spread
(max - min).

    python tools/bench_generate.py [--batch 1,16] [--rounds 5] [--baseline-only] [--out profiles/decode_loop_bench.json]

With --draft-len 0,2,4,7 the tool measures the speculative loop instead (SpecDecodeLoop, qqq_amd/serve.py) and writes
profiles/spec_decode_bench.json: per batch and draft length K the time of one replayed step ((wall time with NEW tokens - wall time with 1
token) / the steps the loop replayed, the same cold protocol; K = 0 is DecodeLoop), r(K) = step time at K over step time at 0, the
break-even mean number of accepted drafts per row-step r(K) - 1, and tokens/s in two regimes: the random model, where next to no draft
comes true (the cost of the wider step, the worst case), and the same model rigged to emit a period of 16 tokens (embeddings scaled up,
lm_head row (t + 1) % 16 set to the embedding of t), where nearly every draft does (the upper bound).  The acceptance itself is measured
and written, not assumed.  Acceptance on real text is not measured: that needs a checkpoint and a tokenizer.

    python tools/bench_generate.py --draft-len 0,2,4,7 [--batch 1,16] [--rounds 5] [--out profiles/spec_decode_bench.json]

With --verify as well, every K > 0 is measured twice in the same rotation: with fuse_prefill() alone (the step's chunk through the paged
prefill attention kernel, the runs above) and with fuse_verify() beside it (the chunk through the verify attention kernel; admission
prefill keeps the prefill kernel).  A loop captures its step under its own flags in the warm-up, and the flags are set again before each
of its runs.  Written to profiles/spec_decode_verify_bench.json: both step times with the rounds' min and max, r(K) before and after, and
the part of the gap to K = 0 that the verify kernel closes.

    python tools/bench_generate.py --draft-len 0,4 --verify [--batch 1,16] [--rounds 5] [--out profiles/spec_decode_verify_bench.json]

With --penalties the tool times the replayed step with and without ops.penalize_logits in it, in one rotation: per batch and draft length
K (default 0,4; 0 is DecodeLoop) a loop built with penalties=True serving generate(repetition_penalty=1.3, presence_penalty=0.5,
frequency_penalty=0.25) beside a loop built without, by the protocol above.  Written to profiles/penalty_loop_bench.json: both step times
with the rounds' min and max, their difference, and whether it exceeds the plain step's own round-to-round spread.  A row's history is
the prompt and what it emitted, 128 ... 255 tokens here; the op's time at longer histories is in profiles/penalty_bench.json
(tools/bench_sample.py --penalties).

    python tools/bench_generate.py --penalties [--draft-len 0,4] [--batch 1,16] [--rounds 5] [--out profiles/penalty_loop_bench.json]

With --logprobs 0,5,20 the tool times the replayed step with and without ops.topk_logprobs_step in it, in one rotation: per batch a
DecodeLoop built without logprobs beside one built with logprobs=k for every k given, by the protocol above.  Written to
profiles/logprobs_loop_bench.json: the step times and each epilogue's difference to the plain step, beside the plain step's spread over
the rounds.  The op alone is in profiles/logprobs_bench.json (tools/bench_sample.py --logprobs).

    python tools/bench_generate.py --logprobs 0,5,20 [--batch 1,16] [--rounds 5] [--out profiles/logprobs_loop_bench.json]

With --stops the tool times the replayed step with and without ops.ban_tokens and ops.stop_check in it, in one rotation: per batch and
draft length K (default 0,4; 0 is DecodeLoop) a loop built with stops=True serving generate(stop=eight 4-token sequences,
stop_token_ids=two ids, min_new_tokens=8) beside a loop built without, by the protocol above, and beside them the plain loop at
sync_every=1 -- a host sync per step, the only way to honour a stop sequence without the two ops.  The stop sequences and ids are
chosen not to occur (every run must emit all its tokens), so all three loops run the same steps.  Written to
profiles/stop_loop_bench.json: the three step times with the rounds' min and max, the ops' difference to the plain step beside the spread
of both runs over the rounds, and what a sync per step costs against it.  No threshold: the feature is opt-in.

    python tools/bench_generate.py --stops [--draft-len 0,4] [--batch 1,16] [--rounds 5] [--out profiles/stop_loop_bench.json]

With --n 1,4,8 the tool measures parallel sampling: per N one prompt of --prompt tokens (default 2048: sixteen 128-key chunks of the decode
plan) served three ways by a captured DecodeLoop in one rotation -- `repeated`: the prompt N times in N rows (N prefills, N copies of its
keys); `forked`: DecodeLoop(family=N) without fuse_shared() (one prefill, the prompt's blocks once, the plain paged decode op over the
aliased tables); `forked_shared`: the same with fuse_shared().  By the protocol above: the time of one replayed step, tokens/s of the N
rows, and the pool blocks in use at the peak (from the allocator; the saving is exact arithmetic and independent of the kernel).  Sampling
at temperature 0.8 so that the siblings diverge.  Written to profiles/parallel_sampling_bench.json.

    python tools/bench_generate.py --n 1,4,8 [--prompt 2048] [--rounds 5] [--out profiles/parallel_sampling_bench.json]

With --lora the tool times the replayed step of a loop built without a LoraBank (`off`), of a loop with one (ops.lora_add behind every
projection: rank 16, every row on slot 0 -- `one` -- and row r on slot r -- `distinct`) and of the same loop with the op replaced by the
torch composition of tools/bench_lora.py (`torch_one`, `torch_distinct`), in one rotation, at K = 0 and 4 (--draft-len), and writes
profiles/lora_loop_bench.json: the step times with the rounds' min and max, what each adds to `off`, the largest spread of the rounds, and
whether the op's addition is below the composition's by more than that spread.

    python tools/bench_generate.py --lora [--batch 1,16] [--draft-len 0,4] [--rounds 5] [--out profiles/lora_loop_bench.json]

With --guided the tool times the replayed step with and without ops.fsm_mask and ops.fsm_advance in it, in one rotation: per batch a plain
DecodeLoop beside a GuidedDecodeLoop serving generate_guided() with one automaton per prompt that allows exactly the plain loop's own
completion (TokenFSM.from_choices of that one sequence: one allowed token per state, so the mask writes the whole row, its dearest case),
by the protocol above.  Both loops emit the same tokens (asserted) and so run the same steps.  Written to
profiles/guided_loop_bench.json: both step times with the rounds' min and max, the ops' difference to the plain step and the spread of
both runs over the rounds.  No threshold: the feature is opt-in.  The ops alone are in profiles/fsm_bench.json (tools/bench_sample.py --fsm).

    python tools/bench_generate.py --guided [--batch 1,16] [--rounds 5] [--out profiles/guided_loop_bench.json]

With --qwen3 the model is four Qwen3-8B-shaped layers (hidden 4096, 32 / 8 heads of 128, intermediate 12288, random q_norm / k_norm) and
the tool times the replayed step of a DecodeLoop three ways in one rotation, by the protocol above: `fused` (ops.rope_qkv_norm_paged, the
per-head norm inside the RoPE / cache-write launch), `composed` (the same loop with that op replaced by Qwen3RMSNorm's torch lines on the
q and k views and ops.rope_qkv_paged) and `no_norm` (the layers with qk_norm off: another function, it shows what the norm costs in a
step).  Written to profiles/qwen3_loop_bench.json: the step times with the rounds' min and max, the two differences, the largest spread
of the rounds, and whether each difference exceeds it.

    python tools/bench_generate.py --qwen3 [--batch 1,16] [--rounds 5] [--out profiles/qwen3_loop_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PROMPT, NEW, BS, LAYERS, SYNC_EVERY = 128, 128, 16, 4, 8


def point(lm, batch, rounds, baseline_only, dev):
    import torch

    from bench_model import VOCAB

    g = torch.Generator().manual_seed(batch)
    prompts = [torch.randint(0, VOCAB, (PROMPT,), generator=g).tolist() for _ in range(batch)]
    blocks = batch * -(-(PROMPT + NEW - 1) // BS)
    base_cache = lm.new_cache(blocks, BS)
    variants = {"generate": lambda n: lm.generate(prompts, n, cache=base_cache)}
    if not baseline_only:
        from qqq_amd import DecodeLoop

        max_len = -(-(PROMPT + NEW - 1) // BS) * BS
        for name, graph in (("loop_eager", False), ("loop_graph", True)):
            loop = DecodeLoop(lm, lm.new_cache(blocks, BS), rows=batch, max_len=max_len, sync_every=SYNC_EVERY, graph=graph)
            variants[name] = lambda n, loop=loop: loop.generate(prompts, n)

    def timed(f, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f(n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    tokens = {}
    for name, f in variants.items():  # warm-up: code objects, workspaces, rope tables, the capture
        timed(f, 1)
        tokens[name] = timed(f, NEW)[1]
        assert all(len(o) == NEW for o in tokens[name]), name
    values, shorts = {name: [] for name in variants}, {name: [] for name in variants}
    for _ in range(rounds):
        for name, f in variants.items():
            short, full = timed(f, 1)[0], timed(f, NEW)[0]
            values[name].append((full - short) / (NEW - 1) * 1e6)
            shorts[name].append(short * 1e6)
    res = {"batch": batch, "prompt_tokens": PROMPT, "new_tokens": NEW, "layers": LAYERS}
    for name, v in values.items():
        res[name] = {"median_us_per_token": round(statistics.median(v), 1), "min_us_per_token": round(min(v), 1),
                     "max_us_per_token": round(max(v), 1), "rounds_us_per_token": [round(x, 1) for x in v],
                     "one_token_us": {"median": round(statistics.median(shorts[name]), 1), "min": round(min(shorts[name]), 1),
                                      "max": round(max(shorts[name]), 1), "rounds": [round(x, 1) for x in shorts[name]]}}
    if not baseline_only:
        assert tokens["loop_graph"] == tokens["loop_eager"], "the captured loop and the eager loop must emit the same tokens"
        # generate's decode batch is sized for the running sequences' lengths, the loop's for max_len: another split plan, so the last
        # bits of the attention output, and with them a greedy token, may differ
        res["loop_tokens_equal_generate"] = tokens["loop_graph"] == tokens["generate"]
        base, graph = res["generate"], res["loop_graph"]
        res["generate_over_loop_graph"] = round(base["median_us_per_token"] / graph["median_us_per_token"], 2)
        res["generate_round_spread_us"] = round(base["max_us_per_token"] - base["min_us_per_token"], 1)
        res["loop_graph_below_generate_by_more_than_its_spread"] = bool(
            graph["median_us_per_token"] < base["median_us_per_token"] - res["generate_round_spread_us"])
    return res


PERIOD, RIG_SCALE = 16, 8.0


def rig(lm):
    """Make the model emit the period 0, 1, ... PERIOD - 1: the embeddings dominate the residual stream, and the head's row (t + 1) % PERIOD
    is the embedding of t (every other row 0).  In place: captured graphs keep their addresses."""
    emb = lm.model.embed_tokens.weight.data
    emb.mul_(RIG_SCALE)
    head = lm.lm_head.weight.data
    head.zero_()
    for t in range(PERIOD):
        head[(t + 1) % PERIOD].copy_(emb[t] / RIG_SCALE)


def spec_point(lm, batch, drafts, rounds, rigged, dev, verify=False):
    import torch

    from bench_model import VOCAB
    from qqq_amd import DecodeLoop, SpecDecodeLoop

    g = torch.Generator().manual_seed(batch)
    if rigged:
        prompts = [[(s + i) % PERIOD for i in range(PROMPT)] for s in range(batch)]
    else:
        prompts = [torch.randint(0, VOCAB, (PROMPT,), generator=g).tolist() for _ in range(batch)]
    loops = {}  # key: K, or "Kv" for the loop whose step takes the verify kernel
    for k in drafts:
        max_len = -(-(PROMPT + NEW - 1 + k) // BS) * BS
        for key in ([k, f"{k}v"] if verify and k else [k]):
            cache = lm.new_cache(batch * (max_len // BS), BS)
            loops[key] = (SpecDecodeLoop(lm, cache, rows=batch, max_len=max_len, draft_len=k, sync_every=SYNC_EVERY) if k else
                          DecodeLoop(lm, cache, rows=batch, max_len=max_len, sync_every=SYNC_EVERY))
            loops[key].verify = isinstance(key, str)

    def timed(loop, n):
        (lm.fuse_verify if loop.verify else lm.unfuse_verify)()  # the eager parts follow the flags of the run; the capture is the warm-up's
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loop.generate(prompts, n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    stats, tokens = {}, {}
    for k, loop in loops.items():  # warm-up: code objects, workspaces, rope tables, the capture
        timed(loop, 1)
        out = tokens[str(k)] = timed(loop, NEW)[1]
        assert all(len(o) == NEW for o in out), k
        steps = loop.steps if k else NEW - 1
        stats[k] = {"steps": steps, "row_steps": loop.row_steps if k else batch * (NEW - 1), "accepted": loop.accepted if k else 0}
    values = {k: [] for k in loops}
    for _ in range(rounds):
        for k, loop in loops.items():
            short, full = timed(loop, 1)[0], timed(loop, NEW)[0]
            values[k].append(full - short)
    res = {"batch": batch, "model": "rigged to a period" if rigged else "random", "prompt_tokens": PROMPT, "new_tokens": NEW, "layers": LAYERS,
           "draft_len": {}}
    for k, v in values.items():
        sec, st = statistics.median(v), stats[k]
        res["draft_len"][str(k)] = {
            "steps": st["steps"], "accepted_per_row_step": round(st["accepted"] / max(st["row_steps"], 1), 3),
            "step_us": round(sec / st["steps"] * 1e6, 1), "step_us_min": round(min(v) / st["steps"] * 1e6, 1),
            "step_us_max": round(max(v) / st["steps"] * 1e6, 1), "tokens_per_s": round(batch * (NEW - 1) / sec, 1),
            "rounds_ms": [round(x * 1e3, 2) for x in v]}
    base = res["draft_len"].get("0")
    if base:
        for k, e in res["draft_len"].items():
            e["r"] = round(e["step_us"] / base["step_us"], 3)
            e["break_even_accepted_per_row_step"] = round(e["r"] - 1, 3)
            e["tokens_per_s_over_draft_len_0"] = round(e["tokens_per_s"] / base["tokens_per_s"], 3)
        for k, e in res["draft_len"].items():
            if k.endswith("v"):  # the verify kernel against the prefill kernel at the same K, timed in the same rotation
                before = res["draft_len"][k[:-1]]
                gap = before["step_us"] - base["step_us"]
                e["attention"], before["attention"] = "verify_attention_paged", "prefill_attention_paged"
                e["step_us_saved"] = round(before["step_us"] - e["step_us"], 1)
                e["prefill_path_round_spread_us"] = round(before["step_us_max"] - before["step_us_min"], 1)
                e["share_of_gap_to_draft_len_0_closed"] = round(e["step_us_saved"] / gap, 3) if gap > 0 else None
                e["tokens_equal_prefill_path"] = tokens[k] == tokens[k[:-1]]
    return res


def spec_main(args):
    import torch

    from bench_model import build

    drafts = sorted({int(k) for k in args.draft_len.split(",")})
    dev = torch.device("cuda:0")
    lm = build(LAYERS, dev).fuse_prefill()
    batches = list(map(int, args.batch.split(",")))
    with torch.no_grad():
        points = [spec_point(lm, b, drafts, args.rounds, False, dev, args.verify) for b in batches]
        rig(lm)
        points += [spec_point(lm, b, drafts, args.rounds, True, dev, args.verify) for b in batches]
    lm.unfuse_verify()
    out = {"tool": "tools/bench_generate.py --draft-len " + args.draft_len + (" --verify" if args.verify else ""),
           "device": torch.cuda.get_device_name(0),
           "shape": "Llama-2-7B layers, per-channel W4A8, fuse_qkv(), fuse_prefill(), paged fp16 cache, block 16, greedy, ngram_max 3",
           "sync_every": SYNC_EVERY, "rounds": args.rounds,
           "not_measured": "acceptance on real text: no checkpoint or tokenizer was available; the two models bracket it", "points": points}
    path = args.out or os.path.join(ROOT, "profiles", "spec_decode_verify_bench.json" if args.verify else "spec_decode_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"batch {p['batch']:3d} {p['model']}: " + "  ".join(
            f"K={k} {e['step_us']:.0f} us/step r={e.get('r')} acc={e['accepted_per_row_step']} {e['tokens_per_s']:.0f} tok/s"
            for k, e in p["draft_len"].items()))


PENALTIES = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25)


def penalty_point(lm, batch, drafts, rounds, dev):
    import torch

    from bench_model import VOCAB
    from qqq_amd import DecodeLoop, SpecDecodeLoop

    g = torch.Generator().manual_seed(batch)
    prompts = [torch.randint(0, VOCAB, (PROMPT,), generator=g).tolist() for _ in range(batch)]
    loops = {}  # key: (K, with the op)
    for k in drafts:
        max_len = -(-(PROMPT + NEW - 1 + k) // BS) * BS
        for on in (False, True):
            cache = lm.new_cache(batch * (max_len // BS), BS)
            kw = dict(rows=batch, max_len=max_len, sync_every=SYNC_EVERY, **(dict(penalties=True) if on else {}))
            loops[(k, on)] = SpecDecodeLoop(lm, cache, draft_len=k, **kw) if k else DecodeLoop(lm, cache, **kw)

    def timed(key, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loops[key].generate(prompts, n, **(PENALTIES if key[1] else {}))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    steps = {}
    for key, loop in loops.items():  # warm-up: code objects, workspaces, rope tables, the capture
        timed(key, 1)
        assert all(len(o) == NEW for o in timed(key, NEW)[1]), key
        steps[key] = loop.steps if key[0] else NEW - 1
    values = {key: [] for key in loops}
    for _ in range(rounds):
        for key in loops:
            short, full = timed(key, 1)[0], timed(key, NEW)[0]
            values[key].append((full - short) / steps[key] * 1e6)
    res = {"batch": batch, "prompt_tokens": PROMPT, "new_tokens": NEW, "layers": LAYERS, "draft_len": {}}
    for k in drafts:
        e = {}
        for on, name in ((False, "plain"), (True, "penalised")):
            v = values[(k, on)]
            e[name] = {"steps": steps[(k, on)], "step_us": round(statistics.median(v), 1), "step_us_min": round(min(v), 1),
                       "step_us_max": round(max(v), 1), "rounds_step_us": [round(x, 1) for x in v]}
        e["op_us_per_step"] = round(e["penalised"]["step_us"] - e["plain"]["step_us"], 1)
        e["plain_round_spread_us"] = round(e["plain"]["step_us_max"] - e["plain"]["step_us_min"], 1)
        e["op_exceeds_the_plain_steps_spread"] = bool(e["op_us_per_step"] > e["plain_round_spread_us"])
        res["draft_len"][str(k)] = e
    return res


def penalty_main(args):
    import torch

    from bench_model import build

    drafts = sorted({int(k) for k in (args.draft_len or "0,4").split(",")})
    dev = torch.device("cuda:0")
    lm = build(LAYERS, dev).fuse_prefill()
    with torch.no_grad():
        points = [penalty_point(lm, b, drafts, args.rounds, dev) for b in map(int, args.batch.split(","))]
    out = {"tool": "tools/bench_generate.py --penalties", "device": torch.cuda.get_device_name(0),
           "shape": "Llama-2-7B layers, per-channel W4A8, fuse_qkv(), fuse_prefill(), paged fp16 cache, block 16, greedy, ngram_max 3",
           "penalties": PENALTIES, "history_tokens": [PROMPT, PROMPT + NEW - 1], "sync_every": SYNC_EVERY, "rounds": args.rounds,
           "points": points}
    path = args.out or os.path.join(ROOT, "profiles", "penalty_loop_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"batch {p['batch']:3d}: " + "  ".join(
            f"K={k} plain {e['plain']['step_us']:.1f} penalised {e['penalised']['step_us']:.1f} us/step (+{e['op_us_per_step']}, plain spread "
            f"{e['plain_round_spread_us']})" for k, e in p["draft_len"].items()))


def logprobs_point(lm, batch, ks, rounds, dev):
    import torch

    from bench_model import VOCAB
    from qqq_amd import DecodeLoop

    g = torch.Generator().manual_seed(batch)
    prompts = [torch.randint(0, VOCAB, (PROMPT,), generator=g).tolist() for _ in range(batch)]
    max_len = -(-(PROMPT + NEW - 1) // BS) * BS
    loops = {}  # key: None (the plain loop) or k
    for k in [None] + ks:
        kw = dict(rows=batch, max_len=max_len, sync_every=SYNC_EVERY, **({} if k is None else dict(logprobs=k)))
        loops[k] = DecodeLoop(lm, lm.new_cache(batch * (max_len // BS), BS), **kw)

    def timed(key, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loops[key].generate(prompts, n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, (out if key is None else out[0])

    tokens = {}
    for key in loops:  # warm-up: code objects, workspaces, rope tables, the capture
        timed(key, 1)
        tokens[key] = timed(key, NEW)[1]
        assert all(len(o) == NEW for o in tokens[key]) and tokens[key] == tokens[None], key
    values = {key: [] for key in loops}
    for _ in range(rounds):
        for key in loops:
            short, full = timed(key, 1)[0], timed(key, NEW)[0]
            values[key].append((full - short) / (NEW - 1) * 1e6)
    res = {"batch": batch, "prompt_tokens": PROMPT, "new_tokens": NEW, "layers": LAYERS, "vocab": VOCAB, "logprobs": {}}

    def entry(v):
        return {"step_us": round(statistics.median(v), 1), "step_us_min": round(min(v), 1), "step_us_max": round(max(v), 1),
                "rounds_step_us": [round(x, 1) for x in v]}

    res["plain"] = entry(values[None])
    res["plain_round_spread_us"] = round(res["plain"]["step_us_max"] - res["plain"]["step_us_min"], 1)
    for k in ks:
        e = entry(values[k])
        e["epilogue_us_per_step"] = round(e["step_us"] - res["plain"]["step_us"], 1)
        e["epilogue_exceeds_the_plain_steps_spread"] = bool(e["epilogue_us_per_step"] > res["plain_round_spread_us"])
        res["logprobs"][str(k)] = e
    return res


def logprobs_main(args):
    import torch

    from bench_model import build

    ks = sorted({int(k) for k in args.logprobs.split(",")})
    dev = torch.device("cuda:0")
    lm = build(LAYERS, dev)
    with torch.no_grad():
        points = [logprobs_point(lm, b, ks, args.rounds, dev) for b in map(int, args.batch.split(","))]
    out = {"tool": "tools/bench_generate.py --logprobs", "device": torch.cuda.get_device_name(0),
           "shape": "Llama-2-7B layers, per-channel W4A8, fuse_qkv(), paged fp16 cache, block 16, greedy", "sync_every": SYNC_EVERY,
           "rounds": args.rounds, "points": points}
    path = args.out or os.path.join(ROOT, "profiles", "logprobs_loop_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"batch {p['batch']:3d}: plain {p['plain']['step_us']:.1f} us/step (spread {p['plain_round_spread_us']})  " + "  ".join(
            f"k={k} {e['step_us']:.1f} (+{e['epilogue_us_per_step']})" for k, e in p["logprobs"].items()))


def stops_point(lm, batch, drafts, rounds, dev):
    import torch

    from bench_model import VOCAB
    from qqq_amd import DecodeLoop, SpecDecodeLoop

    g = torch.Generator().manual_seed(batch)
    prompts = [torch.randint(0, VOCAB, (PROMPT,), generator=g).tolist() for _ in range(batch)]
    loops = {}  # key: (K, "plain" | "stops" | "sync1")
    for k in drafts:
        max_len = -(-(PROMPT + NEW - 1 + k) // BS) * BS
        for name in ("plain", "stops", "sync1"):
            cache = lm.new_cache(batch * (max_len // BS), BS)
            kw = dict(rows=batch, max_len=max_len, sync_every=1 if name == "sync1" else SYNC_EVERY, **(dict(stops=True) if name == "stops" else {}))
            loops[(k, name)] = SpecDecodeLoop(lm, cache, draft_len=k, **kw) if k else DecodeLoop(lm, cache, **kw)

    free = loops[(drafts[0], "plain")].generate(prompts, NEW)
    emitted = {t for o in free for t in o}
    unused = [t for t in range(VOCAB) if t not in emitted]  # the speculative loop may leave the plain loop's tokens at a near-tie: asserted below
    stops = dict(stop=[unused[4 * i:4 * i + 4] for i in range(8)], stop_token_ids=unused[32:34], min_new_tokens=8)

    def timed(key, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loops[key].generate(prompts, n, **(stops if key[1] == "stops" else {}))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    steps = {}
    for key, loop in loops.items():  # warm-up: code objects, workspaces, rope tables, the capture
        timed(key, 1)
        assert all(len(o) == NEW for o in timed(key, NEW)[1]), key  # no stop occurred: the loops ran the same steps
        steps[key] = loop.steps if key[0] else NEW - 1
    values = {key: [] for key in loops}
    for _ in range(rounds):
        for key in loops:
            short, full = timed(key, 1)[0], timed(key, NEW)[0]
            values[key].append((full - short) / steps[key] * 1e6)
    res = {"batch": batch, "prompt_tokens": PROMPT, "new_tokens": NEW, "layers": LAYERS, "draft_len": {}}
    for k in drafts:
        e = {}
        for name in ("plain", "stops", "sync1"):
            v = values[(k, name)]
            e[name] = {"steps": steps[(k, name)], "sync_every": 1 if name == "sync1" else SYNC_EVERY, "step_us": round(statistics.median(v), 1),
                       "step_us_min": round(min(v), 1), "step_us_max": round(max(v), 1), "rounds_step_us": [round(x, 1) for x in v]}
        e["ops_us_per_step"] = round(e["stops"]["step_us"] - e["plain"]["step_us"], 1)
        e["plain_round_spread_us"] = round(e["plain"]["step_us_max"] - e["plain"]["step_us_min"], 1)
        e["stops_round_spread_us"] = round(e["stops"]["step_us_max"] - e["stops"]["step_us_min"], 1)
        e["ops_exceed_both_spreads"] = bool(e["ops_us_per_step"] > max(e["plain_round_spread_us"], e["stops_round_spread_us"]))
        e["sync_per_step_us_over_plain"] = round(e["sync1"]["step_us"] - e["plain"]["step_us"], 1)
        res["draft_len"][str(k)] = e
    return res


def stops_main(args):
    import torch

    from bench_model import build

    drafts = sorted({int(k) for k in (args.draft_len or "0,4").split(",")})
    dev = torch.device("cuda:0")
    lm = build(LAYERS, dev).fuse_prefill()
    with torch.no_grad():
        points = [stops_point(lm, b, drafts, args.rounds, dev) for b in map(int, args.batch.split(","))]
    out = {"tool": "tools/bench_generate.py --stops", "device": torch.cuda.get_device_name(0),
           "shape": "Llama-2-7B layers, per-channel W4A8, fuse_qkv(), fuse_prefill(), paged fp16 cache, block 16, greedy, ngram_max 3",
           "stops": "eight 4-token stop sequences, two stop token ids, min_new_tokens 8; none occurs", "sync_every": SYNC_EVERY,
           "rounds": args.rounds, "points": points}
    path = args.out or os.path.join(ROOT, "profiles", "stop_loop_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"batch {p['batch']:3d}: " + "  ".join(
            f"K={k} plain {e['plain']['step_us']:.1f} stops {e['stops']['step_us']:.1f} us/step (+{e['ops_us_per_step']}, spreads "
            f"{e['plain_round_spread_us']} / {e['stops_round_spread_us']}) sync_every=1 {e['sync1']['step_us']:.1f}" for k, e in p["draft_len"].items()))


def guided_point(lm, batch, rounds, dev):
    import torch

    from bench_model import VOCAB
    from qqq_amd import DecodeLoop, GuidedDecodeLoop, TokenFSM

    g = torch.Generator().manual_seed(batch)
    prompts = [torch.randint(0, VOCAB, (PROMPT,), generator=g).tolist() for _ in range(batch)]
    max_len = -(-(PROMPT + NEW - 1) // BS) * BS
    room = 1 << (batch * (NEW + 1) - 1).bit_length()
    loops = {"plain": DecodeLoop(lm, lm.new_cache(batch * (max_len // BS), BS), rows=batch, max_len=max_len, sync_every=SYNC_EVERY),
             "guided": GuidedDecodeLoop(lm, lm.new_cache(batch * (max_len // BS), BS), rows=batch, max_len=max_len, sync_every=SYNC_EVERY,
                                        fsm_states=room, fsm_edges=room)}
    free = loops["plain"].generate(prompts, NEW)
    fsms = [TokenFSM.from_choices([o], vocab=VOCAB) for o in free]  # the plain loop's own completions: the same steps, one allowed token each

    def timed(name, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loops[name].generate(prompts, n) if name == "plain" else loops[name].generate_guided(prompts, fsms, n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for name in loops:  # warm-up: code objects, workspaces, rope tables, the capture
        timed(name, 1)
        assert timed(name, NEW)[1] == free, name
    values = {name: [] for name in loops}
    for _ in range(rounds):
        for name in loops:
            short, full = timed(name, 1)[0], timed(name, NEW)[0]
            values[name].append((full - short) / (NEW - 1) * 1e6)
    res = {"batch": batch, "prompt_tokens": PROMPT, "new_tokens": NEW, "layers": LAYERS, "fsm_states": sum(f.n_states for f in fsms),
           "fsm_capacity": room}
    for name, v in values.items():
        res[name] = {"sync_every": SYNC_EVERY, "step_us": round(statistics.median(v), 1), "step_us_min": round(min(v), 1),
                     "step_us_max": round(max(v), 1), "rounds_step_us": [round(x, 1) for x in v]}
    res["ops_us_per_step"] = round(res["guided"]["step_us"] - res["plain"]["step_us"], 1)
    res["plain_round_spread_us"] = round(res["plain"]["step_us_max"] - res["plain"]["step_us_min"], 1)
    res["guided_round_spread_us"] = round(res["guided"]["step_us_max"] - res["guided"]["step_us_min"], 1)
    res["ops_exceed_both_spreads"] = bool(res["ops_us_per_step"] > max(res["plain_round_spread_us"], res["guided_round_spread_us"]))
    return res


def guided_main(args):
    import torch

    from bench_model import build

    dev = torch.device("cuda:0")
    lm = build(LAYERS, dev).fuse_prefill()
    with torch.no_grad():
        points = [guided_point(lm, b, args.rounds, dev) for b in map(int, args.batch.split(","))]
    out = {"tool": "tools/bench_generate.py --guided", "device": torch.cuda.get_device_name(0),
           "shape": "Llama-2-7B layers, per-channel W4A8, fuse_qkv(), fuse_prefill(), paged fp16 cache, block 16, greedy",
           "automaton": "per prompt the chain of the plain loop's own completion: one allowed token per state", "sync_every": SYNC_EVERY,
           "rounds": args.rounds, "points": points}
    path = args.out or os.path.join(ROOT, "profiles", "guided_loop_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"batch {p['batch']:3d}: plain {p['plain']['step_us']:.1f} guided {p['guided']['step_us']:.1f} us/step (+{p['ops_us_per_step']}, spreads "
              f"{p['plain_round_spread_us']} / {p['guided_round_spread_us']})")


def torch_lora_in_step(y, xq, s1, A, B, scale, slot, part_cols=None):
    """what ops.lora_add does, from torch calls that are safe inside a captured step: index_select of A and B by the rows' slots (an idle
    row's -1 reads slot 0 and is scaled by 0), two bmm in f32, scale, and the add into y"""
    import torch

    cols = part_cols if part_cols is not None else (0, y.shape[1])
    idx = slot.clamp_min(0).long()
    R = B.shape[2]
    h = torch.bmm(A.index_select(0, idx).float(), (xq.float() * s1.reshape(-1, 1)).unsqueeze(2))
    sc = (scale.index_select(0, idx) * (slot >= 0))[:, None]
    Bt = B.index_select(0, idx).float()
    for p in range(len(cols) - 1):
        part = y[:, cols[p]:cols[p + 1]]
        part.copy_(part.float() + sc * torch.bmm(Bt[:, cols[p]:cols[p + 1]], h[:, p * R:(p + 1) * R]).squeeze(2))
    return y


def lora_point(lm, bank, batch, drafts, rounds, dev):
    import torch

    from bench_model import VOCAB
    from qqq_amd import DecodeLoop, SpecDecodeLoop, ops

    g = torch.Generator().manual_seed(batch)
    prompts = [torch.randint(0, VOCAB, (PROMPT,), generator=g).tolist() for _ in range(batch)]
    adapters = {"off": None, "one": [0] * batch, "distinct": list(range(batch)), "torch_one": [0] * batch, "torch_distinct": list(range(batch))}
    loops = {}  # key: (K, "off" | "fused" | "torch"); the fused and the torch loop serve "one" and "distinct" each
    for k in drafts:
        max_len = -(-(PROMPT + NEW - 1 + k) // BS) * BS
        for name in ("off", "fused", "torch"):
            kw = dict(rows=batch, max_len=max_len, sync_every=SYNC_EVERY, **({} if name == "off" else dict(lora=bank)))
            cache = lm.new_cache(batch * (max_len // BS), BS)
            loops[(k, name)] = SpecDecodeLoop(lm, cache, draft_len=k, **kw) if k else DecodeLoop(lm, cache, **kw)
    loop_of = {"off": "off", "one": "fused", "distinct": "fused", "torch_one": "torch", "torch_distinct": "torch"}
    fused_op = ops.lora_add

    def timed(k, variant, n):
        ops.lora_add = torch_lora_in_step if loop_of[variant] == "torch" else fused_op  # the torch loop's capture and prefill take the composition
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kw = {} if variant == "off" else dict(adapters=adapters[variant])
            out = loops[(k, loop_of[variant])].generate(prompts, n, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out
        finally:
            ops.lora_add = fused_op

    steps = {}
    for k in drafts:
        for variant in adapters:  # warm-up: code objects, workspaces, rope tables, the capture
            timed(k, variant, 1)
            assert all(len(o) == NEW for o in timed(k, variant, NEW)[1]), (k, variant)
            steps[(k, variant)] = loops[(k, loop_of[variant])].steps if k else NEW - 1
    values = {key: [] for key in steps}
    for _ in range(rounds):
        for k, variant in steps:
            short, full = timed(k, variant, 1)[0], timed(k, variant, NEW)[0]
            values[(k, variant)].append((full - short) / steps[(k, variant)] * 1e6)
    res = {"batch": batch, "prompt_tokens": PROMPT, "new_tokens": NEW, "layers": LAYERS, "draft_len": {}}
    for k in drafts:
        e = {}
        for variant in adapters:
            v = values[(k, variant)]
            e[variant] = {"steps": steps[(k, variant)], "step_us": round(statistics.median(v), 1), "step_us_min": round(min(v), 1),
                          "step_us_max": round(max(v), 1), "rounds_step_us": [round(x, 1) for x in v]}
        spread = max(e[v]["step_us_max"] - e[v]["step_us_min"] for v in e)
        e["largest_round_spread_us"] = round(spread, 1)
        for variant in ("one", "distinct"):
            added, torch_added = e[variant]["step_us"] - e["off"]["step_us"], e["torch_" + variant]["step_us"] - e["off"]["step_us"]
            e[variant + "_added_us"], e["torch_" + variant + "_added_us"] = round(added, 1), round(torch_added, 1)
            e[variant + "_below_torch_by_more_than_the_spread"] = bool(torch_added - added > spread)
        res["draft_len"][str(k)] = e
    return res


def lora_main(args):
    import torch

    from bench_model import build
    from qqq_amd import LoraBank

    drafts = sorted({int(k) for k in (args.draft_len or "0,4").split(",")})
    batches = [int(b) for b in args.batch.split(",")]
    dev = torch.device("cuda:0")
    lm = build(LAYERS, dev).fuse_prefill()
    bank = LoraBank(lm, slots=max(batches), rank=16)
    g = torch.Generator(device=dev).manual_seed(1)
    for t in bank._storage:  # every slot a random adapter of the bank's rank
        t.normal_(0, 0.02, generator=g)
    bank.scale.fill_(2.0)
    with torch.no_grad():
        points = [lora_point(lm, bank, b, drafts, args.rounds, dev) for b in batches]
    out = {"tool": "tools/bench_generate.py --lora", "device": torch.cuda.get_device_name(0),
           "shape": "Llama-2-7B layers, per-channel W4A8, fuse_qkv(), fuse_prefill(), paged fp16 cache, block 16, greedy, ngram_max 3",
           "lora": "rank 16 on all seven projections: five ops.lora_add per layer (q|k|v fused, o, gate, up, down); `one`: every row on slot 0, "
                   "`distinct`: row r on slot r; torch_*: the same loop with the op replaced by index_select, two f32 bmm, scale and add; "
                   "`off`: a loop built without a bank", "bank_bytes": bank.nbytes, "sync_every": SYNC_EVERY, "rounds": args.rounds, "points": points}
    path = args.out or os.path.join(ROOT, "profiles", "lora_loop_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        for k, e in p["draft_len"].items():
            print(f"batch {p['batch']:3d} K={k}: off {e['off']['step_us']:.1f}  one {e['one']['step_us']:.1f} (+{e['one_added_us']})  distinct "
                  f"{e['distinct']['step_us']:.1f} (+{e['distinct_added_us']})  torch one +{e['torch_one_added_us']} distinct "
                  f"+{e['torch_distinct_added_us']}  largest spread {e['largest_round_spread_us']} us/step")


def parallel_point(lm, n, prompt_len, rounds, dev):
    import torch

    from bench_model import VOCAB
    from qqq_amd import DecodeLoop

    g = torch.Generator().manual_seed(n)
    prompt = torch.randint(0, VOCAB, (prompt_len,), generator=g).tolist()
    per = -(-(prompt_len + NEW - 1) // BS)
    max_len = per * BS
    peak = {}

    def watched(cache, name):
        peak[name] = 0
        for fn in ("step", "reserve", "fork"):
            def wrapped(*a, _f=getattr(cache, fn), **kw):
                out = _f(*a, **kw)
                peak[name] = max(peak[name], cache.num_blocks - cache.free_blocks)
                return out
            setattr(cache, fn, wrapped)
        return cache

    variants = {}
    loop = DecodeLoop(lm, watched(lm.new_cache(n * per, BS), "repeated"), rows=n, max_len=max_len, sync_every=SYNC_EVERY)
    variants["repeated"] = (False, lambda k, loop=loop: loop.generate([prompt] * n, k, temperature=0.8, generator=gen()))
    for name, fused in (("forked", False), ("forked_shared", True)):
        if n == 1 and fused:
            continue
        (lm.fuse_shared if fused else lm.unfuse_shared)()  # a loop captures its step under its own flag
        loop = DecodeLoop(lm, watched(lm.new_cache(n * per, BS), name), rows=n, max_len=max_len, sync_every=SYNC_EVERY, family=n)
        variants[name] = (fused, lambda k, loop=loop: loop.generate([prompt], k, temperature=0.8, generator=gen()))

    def gen():
        return torch.Generator(device=dev).manual_seed(1234)

    def timed(name, k):
        fused, f = variants[name]
        (lm.fuse_shared if fused else lm.unfuse_shared)()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f(k)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    tokens = {}
    for name in variants:  # warm-up: code objects, workspaces, rope tables, the capture
        timed(name, 1)
        tokens[name] = timed(name, NEW)[1]
    values = {name: [] for name in variants}
    for _ in range(rounds):
        for name in variants:
            short, full = timed(name, 1)[0], timed(name, NEW)[0]
            values[name].append((full - short) / (NEW - 1) * 1e6)
    lm.unfuse_shared()
    res = {"n": n, "prompt_tokens": prompt_len, "new_tokens": NEW, "layers": LAYERS, "block_size": BS,
           "shared_keys": prompt_len // BS * BS}
    for name, v in values.items():
        med = statistics.median(v)
        res[name] = {"median_us_per_step": round(med, 1), "min_us_per_step": round(min(v), 1), "max_us_per_step": round(max(v), 1),
                     "rounds_us_per_step": [round(x, 1) for x in v], "tokens_per_s": round(n * 1e6 / med, 1),
                     "peak_pool_blocks": peak[name]}
    res["blocks_by_arithmetic"] = {"repeated": n * per, "forked": per + (n - 1) * (per - prompt_len // BS)}
    if "forked_shared" in res:
        res["forked_tokens_equal_forked_shared"] = tokens["forked"] == tokens["forked_shared"]
        base, new = res["forked"], res["forked_shared"]
        res["forked_over_forked_shared"] = round(base["median_us_per_step"] / new["median_us_per_step"], 3)
        res["forked_round_spread_us"] = round(base["max_us_per_step"] - base["min_us_per_step"], 1)
        res["shared_faster_by_more_than_the_spread"] = bool(new["median_us_per_step"] < base["median_us_per_step"] - res["forked_round_spread_us"])
    res["repeated_over_forked"] = round(res["repeated"]["median_us_per_step"] / res["forked"]["median_us_per_step"], 3)
    return res


def parallel_main(args):
    import torch

    from bench_model import build

    args.out = args.out or os.path.join(ROOT, "profiles", "parallel_sampling_bench.json")
    dev = torch.device("cuda:0")
    lm = build(LAYERS, dev)
    with torch.no_grad():
        points = [parallel_point(lm, n, args.prompt, args.rounds, dev) for n in map(int, args.n.split(","))]
    out = {"tool": "tools/bench_generate.py --n", "device": torch.cuda.get_device_name(0),
           "shape": "Llama-2-7B layers, per-channel W4A8, fuse_qkv(), paged fp16 cache, block 16, temperature 0.8",
           "sync_every": SYNC_EVERY, "rounds": args.rounds, "points": points}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"n {p['n']:2d}: " + "  ".join(f"{k} {p[k]['median_us_per_step']:.1f} us/step, {p[k]['peak_pool_blocks']} blocks"
                                             for k in ("repeated", "forked", "forked_shared") if k in p))


QWEN3_8B = dict(model_type="qwen3", vocab_size=32000, hidden_size=4096, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
                intermediate_size=12288, num_hidden_layers=LAYERS, rms_norm_eps=1e-6, rope_theta=1000000.0, attention_bias=False,
                tie_word_embeddings=False)  # Qwen3-8B's layer; the vocabulary is the other modes' 32000, not its 151936


def build_qwen3(dev):
    import types

    import torch

    from qqq_amd import QuantLlamaForCausalLM, pack

    lm = QuantLlamaForCausalLM.from_config(types.SimpleNamespace(**QWEN3_8B), -1).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for mod in lm.modules():
        if hasattr(mod, "s_channel"):
            k, n = mod.infeatures, mod.outfeatures
            mod.B.copy_(pack.pack_codes(torch.randint(-7, 8, (k, n), generator=g, dtype=torch.int8, device=dev), False))
            mod.s_channel.copy_(torch.rand((1, n), generator=g, device=dev) * 2e-4 + 1e-5)
    for layer in lm.model.layers:
        for norm in (layer.self_attn.q_norm, layer.self_attn.k_norm):
            norm.weight.data = (1 + 0.3 * torch.randn(norm.weight.shape, generator=g, device=dev)).half()
    lm.model.embed_tokens.weight.data = torch.randn((lm.model.embed_tokens.weight.shape), generator=g, device=dev).half()
    lm.lm_head.weight.data = (0.05 * torch.randn(lm.lm_head.weight.shape, generator=g, device=dev)).half()
    return lm.eval().fuse_qkv()


def torch_qknorm_in_step(plain_op):
    """ops.rope_qkv_norm_paged(_kv8) from torch calls that are safe inside a captured step: Qwen3RMSNorm's lines on the q and k views of
    the fused GEMM output, then the op without the norm"""
    import torch

    def norm(x, w, eps, d):
        rows = x.reshape(x.shape[0], -1, d)
        h = rows.to(torch.float32)
        h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)
        return (w * h.to(x.dtype)).reshape(x.shape[0], -1)

    def composed(q, k, v, q_weight, k_weight, eps, cos, sin, pos, slots, *pools):
        d = q_weight.shape[0]
        return plain_op(norm(q, q_weight, eps, d), norm(k, k_weight, eps, d), v, cos, sin, pos, slots, *pools)

    return composed


def qwen3_point(lm, batch, rounds, dev):
    import torch

    from qqq_amd import DecodeLoop, ops

    vocab = QWEN3_8B["vocab_size"]
    g = torch.Generator().manual_seed(batch)
    prompts = [torch.randint(0, vocab, (PROMPT,), generator=g).tolist() for _ in range(batch)]
    max_len = -(-(PROMPT + NEW - 1) // BS) * BS
    loops = {name: DecodeLoop(lm, lm.new_cache(batch * (max_len // BS), BS), rows=batch, max_len=max_len, sync_every=SYNC_EVERY)
             for name in ("fused", "composed", "no_norm")}
    fused_op = ops.rope_qkv_norm_paged
    composed_op = torch_qknorm_in_step(ops.rope_qkv_paged)

    def timed(name, n):
        # a loop captures its step in the warm-up under its own variant; the eager prefill of every run follows the same switch
        ops.rope_qkv_norm_paged = composed_op if name == "composed" else fused_op
        for layer in lm.model.layers:
            layer.self_attn.qk_norm = name != "no_norm"
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = loops[name].generate(prompts, n)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out
        finally:
            ops.rope_qkv_norm_paged = fused_op
            for layer in lm.model.layers:
                layer.self_attn.qk_norm = True

    tokens = {}
    for name in loops:  # warm-up: code objects, workspaces, rope tables, the capture
        timed(name, 1)
        tokens[name] = timed(name, NEW)[1]
        assert all(len(o) == NEW for o in tokens[name]), name
    values = {name: [] for name in loops}
    for _ in range(rounds):
        for name in loops:
            short, full = timed(name, 1)[0], timed(name, NEW)[0]
            values[name].append((full - short) / (NEW - 1) * 1e6)
    res = {"batch": batch, "prompt_tokens": PROMPT, "new_tokens": NEW, "layers": LAYERS}
    for name, v in values.items():
        res[name] = {"step_us": round(statistics.median(v), 1), "step_us_min": round(min(v), 1), "step_us_max": round(max(v), 1),
                     "rounds_step_us": [round(x, 1) for x in v]}
    spread = max(res[n]["step_us_max"] - res[n]["step_us_min"] for n in loops)
    res["largest_round_spread_us"] = round(spread, 1)
    res["composed_minus_fused_us_per_step"] = round(res["composed"]["step_us"] - res["fused"]["step_us"], 1)
    res["fused_minus_no_norm_us_per_step"] = round(res["fused"]["step_us"] - res["no_norm"]["step_us"], 1)
    res["fused_below_composed_by_more_than_the_spread"] = bool(res["composed"]["step_us"] - res["fused"]["step_us"] > spread)
    res["norm_cost_exceeds_the_spread"] = bool(res["fused"]["step_us"] - res["no_norm"]["step_us"] > spread)
    res["composed_tokens_equal_fused"] = tokens["composed"] == tokens["fused"]
    return res


def qwen3_main(args):
    import torch

    dev = torch.device("cuda:0")
    lm = build_qwen3(dev).fuse_prefill()
    with torch.no_grad():
        points = [qwen3_point(lm, b, args.rounds, dev) for b in map(int, args.batch.split(","))]
    out = {"tool": "tools/bench_generate.py --qwen3", "device": torch.cuda.get_device_name(0),
           "shape": "Qwen3-8B layers (hidden 4096, 32 / 8 heads of 128, intermediate 12288, q_norm / k_norm), vocabulary 32000, per-channel "
                    "W4A8, fuse_qkv(), fuse_prefill(), paged fp16 cache, block 16, greedy",
           "variants": "`fused`: rope_qkv_norm_paged in the captured step; `composed`: the same loop with the op replaced by Qwen3RMSNorm's "
                       "torch lines on q and k and rope_qkv_paged; `no_norm`: the layers with qk_norm off (another function: what the norm costs)",
           "sync_every": SYNC_EVERY, "rounds": args.rounds, "points": points}
    path = args.out or os.path.join(ROOT, "profiles", "qwen3_loop_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"batch {p['batch']:3d}: fused {p['fused']['step_us']:.1f}  composed {p['composed']['step_us']:.1f}  no norm "
              f"{p['no_norm']['step_us']:.1f} us/step (composed - fused {p['composed_minus_fused_us_per_step']}, fused - no norm "
              f"{p['fused_minus_no_norm_us_per_step']}, largest spread {p['largest_round_spread_us']})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qwen3", action="store_true", help="time the replayed step of four Qwen3-8B-shaped layers with the fused q / k norm op, "
                    "with a torch composition in its place and without the norm (profiles/qwen3_loop_bench.json)")
    ap.add_argument("--n", default=None, help="e.g. 1,4,8: measure parallel sampling instead (profiles/parallel_sampling_bench.json)")
    ap.add_argument("--prompt", type=int, default=2048, help="with --n: tokens of the prompt")
    ap.add_argument("--batch", default="1,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-only", action="store_true", help="time generate() alone (runs on a tree without DecodeLoop)")
    ap.add_argument("--draft-len", default=None, help="e.g. 0,2,4,7: measure the speculative loop instead (profiles/spec_decode_bench.json)")
    ap.add_argument("--verify", action="store_true", help="with --draft-len: every K > 0 also with fuse_verify() "
                    "(profiles/spec_decode_verify_bench.json)")
    ap.add_argument("--penalties", action="store_true", help="time the replayed step with and without ops.penalize_logits "
                    "(profiles/penalty_loop_bench.json)")
    ap.add_argument("--logprobs", default=None, help="e.g. 0,5,20: time the replayed step with and without ops.topk_logprobs_step "
                    "(profiles/logprobs_loop_bench.json)")
    ap.add_argument("--stops", action="store_true", help="time the replayed step with and without ops.ban_tokens and ops.stop_check, and "
                    "the plain loop at sync_every=1 (profiles/stop_loop_bench.json)")
    ap.add_argument("--guided", action="store_true", help="time the replayed step with and without ops.fsm_mask and ops.fsm_advance "
                    "(profiles/guided_loop_bench.json)")
    ap.add_argument("--lora", action="store_true", help="time the replayed step without a LoraBank, with ops.lora_add and with a torch "
                    "composition in its place (profiles/lora_loop_bench.json); --draft-len picks the K, default 0,4")
    ap.add_argument("--out", default=None, help="default profiles/decode_loop_bench.json, or profiles/spec_decode_bench.json with --draft-len")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_generate.py needs a GPU: a timing taken elsewhere says nothing")
    if args.qwen3:
        return qwen3_main(args)
    if args.n:
        return parallel_main(args)
    if args.penalties:
        return penalty_main(args)
    if args.logprobs:
        return logprobs_main(args)
    if args.stops:
        return stops_main(args)
    if args.lora:
        return lora_main(args)
    if args.guided:
        return guided_main(args)
    if args.draft_len:
        return spec_main(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "decode_loop_bench.json")
    from bench_model import build

    dev = torch.device("cuda:0")
    lm = build(LAYERS, dev)
    with torch.no_grad():
        points = [point(lm, b, args.rounds, args.baseline_only, dev) for b in map(int, args.batch.split(","))]
    out = {"tool": "tools/bench_generate.py", "device": torch.cuda.get_device_name(0),
           "shape": "Llama-2-7B layers, per-channel W4A8, fuse_qkv(), paged fp16 cache, block 16, greedy", "sync_every": SYNC_EVERY,
           "rounds": args.rounds, "points": points}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"batch {p['batch']:3d}: " + "  ".join(f"{n} {p[n]['median_us_per_token']:.1f} us/token" for n in
                                                     ("generate", "loop_eager", "loop_graph") if n in p)
              + (f"  | generate / loop graph {p['generate_over_loop_graph']}x, generate's spread {p['generate_round_spread_us']} us"
                 if "generate_over_loop_graph" in p else ""))
    gate = [p for p in points if p["batch"] == 1 and "loop_graph_below_generate_by_more_than_its_spread" in p]
    if gate and not gate[0]["loop_graph_below_generate_by_more_than_its_spread"]:
        sys.exit("batch 1: the captured loop is not below generate() by more than generate()'s spread: the capture is not holding")


if __name__ == "__main__":
    main()
