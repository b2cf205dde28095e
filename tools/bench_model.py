#!/usr/bin/env python3
"""One decode step of a Llama-2-7B-shaped model of a few layers (hidden 4096, 32 heads of 128, intermediate 11008, vocab 32000, per-channel
W4A8) over a PagedKVCache, logits to tokens included, four ways:

    chained + fused     QuantLlamaForCausalLM.forward (the add that ends a layer left to the next norm launch) + ops.sample_tokens
    chained + torch     the same forward + the torch composition of tools/bench_sample.py
    unchained + fused   embedding, layer.forward per layer (a torch add per layer), the final norm, lm_head + ops.sample_tokens
    unchained + torch   the starting point: neither change
Every variant is captured into a hipGraph once (a decode step at a fixed batch and context: the step's metadata stays as it is) and the four
replays are timed alternately, ROUNDS rounds of CALLS event-timed replays; a round's value is the median of its calls.  The saving of the
deferred residual is (unchained - chained) / layers per layer; the sampler's is torch - fused per step.

    python tools/bench_model.py [--layers 4] [--batch 1,16] [--context 1024] [--out profiles/model_step_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROUNDS, CALLS, WARMUP = 5, 20, 5
HIDDEN, HEADS, INTER, VOCAB = 4096, 32, 11008, 32000
T, K, P = 0.8, 50, 0.9


def build(layers, dev):
    import torch

    from qqq_amd import QuantLlamaForCausalLM, QuantLlamaModel, pack

    lm = QuantLlamaForCausalLM(QuantLlamaModel(VOCAB, layers, HIDDEN, HEADS, HEADS, INTER, -1)).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for mod in lm.modules():
        if hasattr(mod, "s_channel"):
            k, n = mod.infeatures, mod.outfeatures
            mod.B.copy_(pack.pack_codes(torch.randint(-7, 8, (k, n), generator=g, dtype=torch.int8, device=dev), False))
            mod.s_channel.copy_(torch.rand((1, n), generator=g, device=dev) * 2e-4 + 1e-5)
    lm.model.embed_tokens.weight.data = torch.randn((VOCAB, HIDDEN), generator=g, device=dev).half()
    lm.lm_head.weight.data = (0.05 * torch.randn((VOCAB, HIDDEN), generator=g, device=dev)).half()
    return lm.eval().fuse_qkv()


def point(lm, batch, context, dev):
    import torch
    import torch.nn.functional as F

    from bench_sample import capture, time_calls, torch_sample
    from qqq_amd import ops

    layers = len(lm.model.layers)
    bs = 16
    cache = lm.new_cache(batch * -(-(context + 1) // bs), bs)
    for s in range(batch):
        cache.add(s)
    cache.step(list(range(batch)), [context - 1] * batch)  # the history: zeros in the pool, which cost what any values cost
    step = cache.step(list(range(batch)), [1] * batch)
    g = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(0, VOCAB, (batch,), generator=g, device=dev)
    u = torch.rand(batch, generator=g, device=dev)
    Tt, kt, pt = (torch.full((batch,), v, dtype=dt, device=dev) for v, dt in ((T, torch.float32), (K, torch.int32), (P, torch.float32)))

    def chained():
        return lm(ids, cache, step)

    def unchained():
        m = lm.model
        x = m.embed_tokens(ids)
        for layer in m.layers:
            x = layer(x, cache, step)
        y = ops.rmsnorm_quant(x, m.norm.weight, m.norm.variance_epsilon, return_y=True)[2]
        return F.linear(y, lm.lm_head.weight)

    fused = lambda logits: ops.sample_tokens(logits, Tt, kt, pt, u)  # noqa: E731
    plain = lambda logits: torch_sample(logits, T, K, P, u)  # noqa: E731
    variants = {"chained+fused": lambda: fused(chained()), "chained+torch": lambda: plain(chained()),
                "unchained+fused": lambda: fused(unchained()), "unchained+torch": lambda: plain(unchained())}
    with torch.no_grad():
        assert torch.equal(chained(), unchained())
        graphs = {n: capture(f) for n, f in variants.items()}
    for gr in graphs.values():
        for _ in range(WARMUP):
            gr.replay()
    torch.cuda.synchronize()
    rounds = {n: [] for n in graphs}
    for _ in range(ROUNDS):
        for n, gr in graphs.items():
            rounds[n].append(statistics.median(time_calls(gr.replay, CALLS)))
    res = {"batch": batch, "context": context, "layers": layers}
    for n, v in rounds.items():
        res[n] = {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                  "rounds_us": [round(x, 1) for x in v]}
    med = lambda n: res[n]["median_us"]  # noqa: E731
    res["deferred_residual_saves_us_per_layer"] = round((med("unchained+fused") - med("chained+fused")) / layers, 2)
    res["fused_sampler_saves_us_per_step"] = round(med("chained+torch") - med("chained+fused"), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--batch", default="1,16")
    ap.add_argument("--context", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_step_bench.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_model.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    lm = build(args.layers, dev)
    points = [point(lm, b, args.context, dev) for b in map(int, args.batch.split(","))]
    out = {"tool": "tools/bench_model.py", "device": torch.cuda.get_device_name(0), "shape": "Llama-2-7B layers, per-channel W4A8, fuse_qkv()",
           "sampling": {"temperature": T, "top_k": K, "top_p": P}, "rounds": ROUNDS, "calls_per_round": CALLS, "points": points}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"batch {p['batch']:3d} context {p['context']}: " + "  ".join(f"{n} {p[n]['median_us']:.1f} us" for n in
              ("chained+fused", "chained+torch", "unchained+fused", "unchained+torch"))
              + f"  | residual {p['deferred_residual_saves_us_per_layer']} us/layer, sampler {p['fused_sampler_saves_us_per_step']} us/step")


if __name__ == "__main__":
    main()
