#!/usr/bin/env python3
"""Beam search's device parts against what they replace, on the same GPU, by tools/bench_sample.py's protocol (alternated in one process,
ROUNDS rounds of CALLS event-timed calls, a round's value the median of its calls; eager, and replayed from a hipGraph where a graph can
hold it).  The JSON keeps every round and reports the median of rounds with their min / max as the spread.

    step     ops.beam_step(logits, cum, live, B, eos, workspace) -- two launches -- against a torch composition of the same semantics:
             log_softmax of an fp32 copy of [P * B, vocab], the add of cum, topk(2B) over [P, B * vocab], div / mod, the eos mask and a
             second topk(B) for the next beams.  Points: vocab {32000, 128256, 151936} x B {4, 16} x P {1, 16}.
    reorder  PagedKVCache.reorder of one parent taken by all B beams (the partial block copied B - 1 times through ops.copy_blocks, one
             launch per pool table) against the same re-pointing with fork / free (a torch copy_ per pool tensor and fork), 32 layers of
             8 kv heads x 128, fp16 and int8 pools, length 40 of block size 16.  Host time included: both are host-driven, timed with the
             wall clock around a synchronize, eager only.
    pass     one replayed decode pass of four Llama-2-7B-shaped layers (hidden 4096, 32 heads, intermediate 11008, vocab 32000) at B = 4,
             one prompt of 512 keys: the forward alone, forward + beam_step, and beam_step and the reorder on their own.

    python tools/bench_beam.py [--out profiles/beam_bench.json] [--parts step,reorder,pass]
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

from bench_sample import CALLS, ROUNDS, WARMUP, capture, time_calls  # noqa: E402

VOCABS, BEAMS, PROMPTS = (32000, 128256, 151936), (4, 16), (1, 16)


def torch_step(logits, cum, B, eos):
    import torch

    rows, vocab = logits.shape
    P = rows // B
    scores = (torch.log_softmax(logits.float(), dim=-1) + cum[:, None]).view(P, B * vocab)
    top, at = torch.topk(scores, 2 * B, dim=-1)
    parent, token = at // vocab, at % vocab
    keep = torch.where(token == eos, torch.full_like(top, float("-inf")), top)
    nxt, pick = torch.topk(keep, B, dim=-1)  # in candidate order: the scores are sorted already
    return top, parent, token, token.gather(1, pick).view(-1), parent.gather(1, pick).view(-1), nxt.view(-1)


def summary(rounds):
    r = {n: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
             "rounds_us": [round(x, 2) for x in v]} for n, v in rounds.items()}
    return r


def alternate(run):
    import torch

    for f in run.values():
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    rounds = {n: [] for n in run}
    for _ in range(ROUNDS):
        for n, f in run.items():
            rounds[n].append(statistics.median(time_calls(f, CALLS)))
    return summary(rounds)


def step_point(P, B, vocab, dev):
    import torch

    from qqq_amd import ops

    g = torch.Generator(device=dev).manual_seed(vocab + 31 * B + P)
    logits = (4.0 * torch.randn((P * B, vocab), generator=g, device=dev)).half()
    cum = -4.0 * torch.rand(P * B, generator=g, device=dev)
    live = torch.ones(P * B, dtype=torch.int32, device=dev)
    eos = 2
    ws = ops.beam_step_workspace(P * B, B, dev)
    fns = {"fused": lambda: ops.beam_step(logits, cum, live, B, eos, ws), "torch": lambda: torch_step(logits, cum, B, eos)}
    a, b = fns["fused"](), fns["torch"]()
    res = {"prompts": P, "num_beams": B, "vocab": vocab,
           "next_ids_equal_fraction": float((a.next_ids == b[3]).float().mean()),  # f32 log_softmax against the exact sums: near-ties may differ
           "max_score_difference": float((a.cand_score - b[0]).abs().max())}
    for how in ("eager", "graph"):
        r = alternate(fns if how == "eager" else {n: capture(f).replay for n, f in fns.items()})
        r["torch_over_fused"] = round(r["torch"]["median_us"] / r["fused"]["median_us"], 2)
        r["torch_over_fused_range"] = [round(r["torch"]["min_us"] / r["fused"]["max_us"], 2), round(r["torch"]["max_us"] / r["fused"]["min_us"], 2)]
        res[how] = r
    return res


def wall(fn, n):
    import torch

    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e6)
    return out


def reorder_point(B, dtype, dev, layers=32):
    import torch

    from qqq_amd import PagedKVCache

    cache = PagedKVCache(layers, 4 * B + 8, 8, 128, 16, device=dev, dtype=dtype)
    seqs = list(range(B))
    for s in seqs:
        cache.add(s)
    cache.step(seqs, [40] * B)
    turn = [0]

    def reorder():
        cache.reorder(seqs, [0] * B)

    def fork_free():  # what the parent commit offers: the next beams forked from the parent, then the old ones freed
        turn[0] += 1
        new = [("t", turn[0], b) for b in range(B)]
        for s in new:
            cache.fork(seqs[0], s)
        for s in seqs:
            cache.free(s)
        seqs[:] = new

    res = {"num_beams": B, "dtype": str(dtype).replace("torch.", ""), "layers": layers, "length": 40}
    for name, fn in (("reorder", reorder), ("fork_free", fork_free)):
        for _ in range(WARMUP):
            fn()
        res[name] = summary({"wall": [statistics.median(wall(fn, CALLS)) for _ in range(ROUNDS)]})["wall"]
    res["fork_free_over_reorder"] = round(res["fork_free"]["median_us"] / res["reorder"]["median_us"], 2)
    return res


def pass_point(dev, B=4, keys=512):
    import torch

    from types import SimpleNamespace

    from qqq_amd import QuantLlamaForCausalLM, ops

    cfg = SimpleNamespace(vocab_size=32000, hidden_size=4096, num_attention_heads=32, num_key_value_heads=32, intermediate_size=11008,
                          num_hidden_layers=4, rms_norm_eps=1e-6, hidden_act="silu", rope_theta=10000.0, max_position_embeddings=4096,
                          attention_bias=False, mlp_bias=False, tie_word_embeddings=False, pad_token_id=None, model_type="llama")
    lm = QuantLlamaForCausalLM.from_config(cfg, -1).to(dev).eval().fuse_prefill().fuse_decode()
    with torch.no_grad():
        for p in lm.parameters():
            if p.dtype == torch.float16:
                p.copy_(torch.randn(p.shape, device=dev).half() * 0.02)
        cache = lm.new_cache(B * (keys // 16 + 2) + 4, 16)
        seqs = list(range(B))
        for s in seqs:
            cache.add(s)
        cache.step(seqs, [keys] * B)  # the keys are zeros: the kernels' work does not depend on them
        step = cache.step(seqs, [1] * B)
        ids = torch.randint(0, 32000, (B,), device=dev)
        cum = torch.zeros(B, device=dev)
        live = torch.ones(B, dtype=torch.int32, device=dev)
        ws = ops.beam_step_workspace(B, B, dev)
        logits = lm(ids, cache, step)
        fns = {"forward": lambda: lm(ids, cache, step), "forward_and_step": lambda: ops.beam_step(lm(ids, cache, step), cum, live, B, 2, ws),
               "step": lambda: ops.beam_step(logits, cum, live, B, 2, ws)}
        res = {"num_beams": B, "keys": keys, "layers": 4, "graph": alternate({n: capture(f).replay for n, f in fns.items()})}
        fn = lambda: cache.reorder(seqs, [0] * B)  # noqa: E731
        for _ in range(WARMUP):
            fn()
        res["reorder_wall"] = summary({"wall": [statistics.median(wall(fn, CALLS)) for _ in range(ROUNDS)]})["wall"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_bench.json"))
    ap.add_argument("--parts", default="step,reorder,pass")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_beam.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    parts = args.parts.split(",")
    out = {"tool": "tools/bench_beam.py", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_round": CALLS}
    if "step" in parts:
        out["step"] = [step_point(P, B, v, dev) for v in VOCABS for B in BEAMS for P in PROMPTS]
        out["step_notes"] = [f"P={p['prompts']} B={p['num_beams']} vocab={p['vocab']} {how}: the op does not win ({p[how]['torch_over_fused']}x)"
                             for p in out["step"] for how in ("eager", "graph") if p[how]["torch_over_fused_range"][0] <= 1.0] or [
                                 "the op wins at every point, also at the unfavourable ends of both spreads"]
        for p in out["step"]:
            print(f"step P {p['prompts']:2d} B {p['num_beams']:2d} vocab {p['vocab']:6d}: " + "  ".join(
                f"{how} fused {p[how]['fused']['median_us']:8.1f} us torch {p[how]['torch']['median_us']:8.1f} us ({p[how]['torch_over_fused']}x)"
                for how in ("eager", "graph")))
    if "reorder" in parts:
        out["reorder"] = [reorder_point(B, dt, dev) for dt in (torch.float16, torch.int8) for B in BEAMS]
        for p in out["reorder"]:
            print(f"reorder B {p['num_beams']:2d} {p['dtype']:8s}: reorder {p['reorder']['median_us']:8.1f} us  fork/free "
                  f"{p['fork_free']['median_us']:8.1f} us ({p['fork_free_over_reorder']}x)")
    if "pass" in parts:
        out["pass"] = pass_point(dev)
        print("pass: " + "  ".join(f"{n} {v['median_us']:.1f} us" for n, v in out["pass"]["graph"].items())
              + f"  reorder (wall) {out['pass']['reorder_wall']['median_us']:.1f} us")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
