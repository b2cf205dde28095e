#!/usr/bin/env python3
"""gptq_quantize with the fused column sweep (one HIP launch per 128-column block) against the same flow with the sweep composed from
torch calls (fused=False: a handful of launches per weight column, what the reference does), on the same GPU, at Llama-2-7B's linear
shapes, per-channel and g128.  Wall time per call with a synchronise on both sides, and the split of the GPU time into the scale search,
the sweep, the trailing GEMM and the Cholesky chain from events around those sections.

    python tools/bench_gptq.py [--rounds 5] [--out profiles/gptq_bench.json] [--small] [--act-order] [--factor torch,fused] [--hessian torch,fused [--experts]]

--act-order times gptq_quantize_ordered (act-order, and static groups when grouped) instead: fused (ops.gptq_block_cols) against its own
fused=False, and against plain gptq_quantize fused, with the split also showing the one-launch group scales and the permutation gathers;
the default --out is then profiles/gptq_order_bench.json.
--factor torch,fused times gptq_quantize (fused sweep) under each factor of the inverse Hessian instead -- torch's Cholesky chain and
ops.upper_factor, alternating in one process -- with the "cholesky" section of both; the default --out is then
profiles/gptq_factor_bench.json.
--hessian torch,fused times Hessian.add_batch under each accumulator instead -- the reference's f32 steps and ops.hessian_update,
alternating in one process -- at K = 4096 and 11008 with 2048 and 8 x 2048 fp16 tokens per call, 16 calls per Hessian, GPU time between
events; and quantize_model over ONE Llama-2-7B-shaped layer (the reference's 128 calibration sequences of 2048 tokens) under both, with the share of its
time the four Hessians take.  The default --out is then profiles/hessian_bench.json.
--hessian torch,fused --experts times ExpertHessians.add_batch under each accumulator instead -- the per-expert loop of f32 steps, which
reads the routing on the host, and ops.hessian_update_grouped -- and, third, E calls of ops.hessian_update on rows gathered BEFORE the
clock starts (what the gather and the one launch buy over the dense op), alternating in one process: Qwen3-30B-A3B's layer (128 experts,
top-8; n = 2048 with a row per token, n = 768 with a row per pair) and Mixtral's (8 experts, top-2, n = 4096) at 2048 and 16384 tokens
per call under random router logits, 4 calls per timing, GPU time between events.  The default --out is then profiles/moe_hessian_bench.json.

Writes the JSON and prints one line per point.  Nothing asserts a time.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008)]  # [N, K]: q/k/v/o, gate/up, down of Llama-2-7B


class EventTimers:
    """section(name): a pair of events around the section; totals() after a synchronise: GPU milliseconds per name"""

    def __init__(self, torch):
        self.torch, self.pairs = torch, []

    def section(self, name):
        return _Section(self, name)

    def totals(self):
        out = {}
        for name, a, b in self.pairs:
            out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        return out


class _Section:
    def __init__(self, timers, name):
        self.t, self.name = timers, name

    def __enter__(self):
        self.a = self.t.torch.cuda.Event(enable_timing=True)
        self.a.record()

    def __exit__(self, *exc):
        b = self.t.torch.cuda.Event(enable_timing=True)
        b.record()
        self.t.pairs.append((self.name, self.a, b))
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="default profiles/gptq_bench.json, with --act-order profiles/gptq_order_bench.json")
    ap.add_argument("--small", action="store_true", help="one 512 x 512 point: the plumbing alone")
    ap.add_argument("--act-order", action="store_true", help="time gptq_quantize_ordered (act-order + static groups) instead")
    ap.add_argument("--factor", default=None, help="torch,fused: time gptq_quantize under both factors of the inverse Hessian instead")
    ap.add_argument("--hessian", default=None, help="torch,fused: time Hessian.add_batch under both accumulators, and its share of a layer, instead")
    ap.add_argument("--experts", action="store_true", help="with --hessian: time ExpertHessians.add_batch (mixture-of-experts layers) instead")
    args = ap.parse_args()
    if args.hessian is not None:
        if sorted(args.hessian.split(",")) != ["fused", "torch"] or args.act_order or args.factor:
            sys.exit("bench_gptq.py: --hessian takes torch,fused (both, so that they share a run), without --act-order / --factor")
        return experts_main(args) if args.experts else hessian_main(args)
    if args.experts:
        sys.exit("bench_gptq.py: --experts goes with --hessian torch,fused")
    factors = args.factor.split(",") if args.factor else []
    if factors and (args.act_order or sorted(factors) != ["fused", "torch"]):
        sys.exit("bench_gptq.py: --factor takes torch,fused (both, so that they share a run), without --act-order")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "gptq_factor_bench.json" if factors else "gptq_order_bench.json" if args.act_order else "gptq_bench.json")
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_gptq.py needs a GPU")
    from qqq_amd.quant import Hessian, gptq_quantize, gptq_quantize_ordered

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    points = []
    for N, K in ([(512, 512)] if args.small else SHAPES):
        W = (torch.randn((N, K), generator=g, device=dev) * 0.02).half()
        h = Hessian(K, dev)
        for _ in range(4):  # four calibration sequences of 512 correlated rows
            x = torch.randn((512, K), generator=g, device=dev) * (0.2 + 2 * torch.rand(K, generator=g, device=dev))
            h.add_batch(x + 0.3 * x.roll(1, dims=1))
        for gs in (-1, 128) if args.act_order else ():
            point = {"N": N, "K": K, "group_size": gs, "act_order": True, "static_groups": gs != -1}
            weights = {}
            runs = {"fused": lambda t: gptq_quantize_ordered(W, h.H, gs, fused=True, timers=t),
                    "composed": lambda t: gptq_quantize_ordered(W, h.H, gs, fused=False, timers=t),
                    "plain_fused": lambda t: gptq_quantize(W, h.H, gs, fused=True, timers=t)}
            for key, run in runs.items():
                run(None)  # warm-up
                torch.cuda.synchronize()
                wall, split = [], []
                for _ in range(args.rounds):
                    timers = EventTimers(torch)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = run(timers)
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    split.append(timers.totals())
                weights[key] = res.weight
                point[key + "_ms"] = [round(t, 3) for t in wall]
                point[key + "_ms_median"] = round(sorted(wall)[len(wall) // 2], 3)
                point[key + "_split_ms_median"] = {k: round(sorted(s[k] for s in split)[len(split) // 2], 3) for k in split[0]}
            point["same_bits"] = bool(torch.equal(weights["fused"], weights["composed"]))
            spread = max(max(point[k + "_ms"]) - min(point[k + "_ms"]) for k in runs)
            point["spread_ms"] = round(spread, 3)
            point["speedup"] = round(point["composed_ms_median"] / point["fused_ms_median"], 2)
            point["fused_wins_by_more_than_the_spread"] = bool(min(point["composed_ms"]) - max(point["fused_ms"]) > spread)
            point["over_plain_fused"] = round(point["fused_ms_median"] / point["plain_fused_ms_median"], 3)
            print(json.dumps(point))
            points.append(point)
        for gs in (-1, 128) if factors else ():
            point = {"N": N, "K": K, "group_size": gs}
            wall, chol, weights = {f: [] for f in factors}, {f: [] for f in factors}, {}
            for f in factors:
                gptq_quantize(W, h.H, gs, factor=f)  # warm-up
            for _ in range(args.rounds):
                for f in factors:  # alternating: both see the same minutes of the machine
                    timers = EventTimers(torch)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = gptq_quantize(W, h.H, gs, timers=timers, factor=f)
                    torch.cuda.synchronize()
                    wall[f].append((time.perf_counter() - t0) * 1e3)
                    chol[f].append(timers.totals()["cholesky"])
                    weights[f] = res.weight
            for f in factors:
                point[f + "_ms"] = [round(t, 3) for t in wall[f]]
                point[f + "_ms_median"] = round(sorted(wall[f])[len(wall[f]) // 2], 3)
                point[f + "_cholesky_ms"] = [round(t, 3) for t in chol[f]]
                point[f + "_cholesky_ms_median"] = round(sorted(chol[f])[len(chol[f]) // 2], 3)
            spread = max(max(chol[f]) - min(chol[f]) for f in factors)
            point["cholesky_spread_ms"] = round(spread, 3)
            point["cholesky_speedup"] = round(point["torch_cholesky_ms_median"] / point["fused_cholesky_ms_median"], 2)
            point["speedup"] = round(point["torch_ms_median"] / point["fused_ms_median"], 2)
            point["fused_wins_by_more_than_the_spread"] = bool(min(chol["torch"]) - max(chol["fused"]) > spread)
            point["weights_that_differ"] = float((weights["torch"] != weights["fused"]).float().mean())
            print(json.dumps(point))
            points.append(point)
        for gs in () if args.act_order or factors else (-1, 128):
            point = {"N": N, "K": K, "group_size": gs}
            weights = {}
            for fused in (True, False):
                gptq_quantize(W, h.H, gs, fused=fused)  # warm-up
                torch.cuda.synchronize()
                wall, split = [], []
                for _ in range(args.rounds):
                    timers = EventTimers(torch)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = gptq_quantize(W, h.H, gs, fused=fused, timers=timers)
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    split.append(timers.totals())
                weights[fused] = res.weight
                key = "fused" if fused else "composed"
                point[key + "_ms"] = [round(t, 3) for t in wall]
                point[key + "_ms_median"] = round(sorted(wall)[len(wall) // 2], 3)
                point[key + "_split_ms_median"] = {k: round(sorted(s[k] for s in split)[len(split) // 2], 3) for k in split[0]}
            point["same_bits"] = bool(torch.equal(weights[True], weights[False]))
            spread = max(max(point[k + "_ms"]) - min(point[k + "_ms"]) for k in ("fused", "composed"))
            point["spread_ms"] = round(spread, 3)
            point["speedup"] = round(point["composed_ms_median"] / point["fused_ms_median"], 2)
            point["fused_wins_by_more_than_the_spread"] = bool(min(point["composed_ms"]) - max(point["fused_ms"]) > spread)
            print(json.dumps(point))
            points.append(point)
        del h
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "points": points}, f, indent=1)
        f.write("\n")


def _median(v):
    return sorted(v)[len(v) // 2]


def hessian_main(args):
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_gptq.py needs a GPU")
    from types import SimpleNamespace

    from qqq_amd.quant import Hessian, quantize_model

    out = args.out or os.path.join(ROOT, "profiles", "hessian_bench.json")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    kinds, calls, points = ("torch", "fused"), 16, []
    for K, seqs in [(256, 1)] if args.small else [(4096, 1), (4096, 8), (11008, 1), (11008, 8)]:
        x = (torch.randn((seqs, 256 if args.small else 2048, K), generator=g, device=dev) * (0.2 + 2 * torch.rand(K, generator=g, device=dev))).half()
        ms, hs = {k: [] for k in kinds}, {}
        for rnd in range(args.rounds + 1):  # (round 0 warms up)
            for k in kinds:  # alternating: both see the same minutes of the machine
                h = Hessian(K, dev, k)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    h.add_batch(x)
                b.record()
                torch.cuda.synchronize()
                if rnd:
                    ms[k].append(a.elapsed_time(b))
                hs[k] = h.H
        point = {"K": K, "tokens_per_call": x.shape[0] * x.shape[1], "calls": calls}
        for k in kinds:
            point[k + "_ms"] = [round(t, 3) for t in ms[k]]
            point[k + "_ms_median"] = round(_median(ms[k]), 3)
        spread = max(max(ms[k]) - min(ms[k]) for k in kinds)
        point["spread_ms"] = round(spread, 3)
        point["speedup"] = round(point["torch_ms_median"] / point["fused_ms_median"], 2)
        point["fused_wins_by_more_than_the_spread"] = bool(min(ms["torch"]) - max(ms["fused"]) > spread)
        point["fused_tflops"] = round(2.0 * calls * point["tokens_per_call"] * K * K / (point["fused_ms_median"] * 1e-3) / 1e12, 1)  # of the full, unhalved product
        point["relative_difference"] = float((hs["fused"].double() - hs["torch"].double()).norm() / hs["torch"].double().norm())
        print(json.dumps(point))
        points.append(point)
        del x, hs, h

    # one layer of Llama-2-7B's shape through quantize_model: what share of it the four Hessians are
    hid, inter, heads, vocab, nseq, seqlen = (256, 512, 4, 1000, 4, 128) if args.small else (4096, 11008, 32, 1000, 128, 2048)
    cfg = SimpleNamespace(model_type="llama", vocab_size=vocab, hidden_size=hid, num_attention_heads=heads, num_key_value_heads=heads,
                          intermediate_size=inter, num_hidden_layers=1, rms_norm_eps=1e-6, rope_theta=10000.0)
    sd = {"model.embed_tokens.weight": torch.randn((vocab, hid), generator=g, device=dev).half(), "model.norm.weight": torch.ones(hid).half(),
          "lm_head.weight": (0.2 * torch.randn((vocab, hid), generator=g, device=dev)).half()}
    for name, (n, k) in {"self_attn.q_proj": (hid, hid), "self_attn.k_proj": (hid, hid), "self_attn.v_proj": (hid, hid), "self_attn.o_proj": (hid, hid),
                         "mlp.gate_proj": (inter, hid), "mlp.up_proj": (inter, hid), "mlp.down_proj": (hid, inter)}.items():
        sd[f"model.layers.0.{name}.weight"] = (torch.randn((n, k), generator=g, device=dev) * k ** -0.5).half()
    for name in ("input_layernorm", "post_attention_layernorm"):
        sd[f"model.layers.0.{name}.weight"] = torch.ones(hid).half()
    ids = torch.randint(0, vocab, (nseq, seqlen), generator=torch.Generator().manual_seed(1))
    timers, plain = None, Hessian.add_batch

    def timed(self, x):
        with timers.section("hessian"):
            plain(self, x)

    Hessian.add_batch = timed
    total, hess = {k: [] for k in kinds}, {k: [] for k in kinds}
    try:
        for rnd in range(args.rounds + 1):
            for k in kinds:
                timers = EventTimers(torch)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                quantize_model(sd, cfg, ids, 128, device=dev, hessian=k)
                b.record()
                torch.cuda.synchronize()
                if rnd:
                    total[k].append(a.elapsed_time(b))
                    hess[k].append(timers.totals()["hessian"])
    finally:
        Hessian.add_batch = plain
    layer = {"hidden": hid, "intermediate": inter, "sequences": nseq, "seqlen": seqlen, "group_size": 128}
    for k in kinds:
        t, h = _median(total[k]), _median(hess[k])
        layer[k] = {"layer_ms": [round(v, 1) for v in total[k]], "hessian_ms": [round(v, 1) for v in hess[k]], "layer_ms_median": round(t, 1),
                    "hessian_ms_median": round(h, 1), "hessian_share": round(h / t, 3)}
    print(json.dumps(layer))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "points": points, "layer": layer}, f, indent=1)
        f.write("\n")


def experts_main(args):
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_gptq.py needs a GPU")
    from qqq_amd import ops as serve_ops
    from qqq_amd.quant import ExpertHessians, ops

    out = args.out or os.path.join(ROOT, "profiles", "moe_hessian_bench.json")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    kinds, calls, points = ("torch", "fused", "dense_calls"), 4, []
    shapes = [("small", 8, 2, 256, 2, 512)] if args.small else [
        (name, E, k, n, a_div, tokens) for name, E, k, n, a_div in (("Qwen3-30B-A3B gate|up", 128, 8, 2048, 8), ("Qwen3-30B-A3B down", 128, 8, 768, 1),
                                                                   ("Mixtral gate|up", 8, 2, 4096, 2)) for tokens in (2048, 16384)]
    for name, E, k, n, a_div, tokens in shapes:
        logits = torch.randn((tokens, E), generator=g, device=dev).half()
        _, _, offsets, order = serve_ops.moe_route(logits, k, True)
        x = (torch.randn((tokens * k // a_div, n), generator=g, device=dev) * (0.2 + 2 * torch.rand(n, generator=g, device=dev))).half()
        offs = offsets.tolist()
        rows = [x[order[offs[e]:offs[e + 1]].long() // a_div].contiguous() for e in range(E)]  # the dense calls' inputs: gathered off the clock
        ms, hs = {kind: [] for kind in kinds}, {}
        for rnd in range(args.rounds + 1):  # (round 0 warms up)
            for kind in kinds:  # alternating: all see the same minutes of the machine
                h = ExpertHessians(E, n, dev, "torch" if kind == "torch" else "fused")
                seen = [0] * E
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    if kind != "dense_calls":
                        h.add_batch(x, offsets, order, a_div)
                        continue
                    for e, r in enumerate(rows):
                        if r.shape[0]:
                            ops.hessian_update(h.H[e], r, seen[e] / (seen[e] + r.shape[0]), 2 / (seen[e] + r.shape[0]))
                            seen[e] += r.shape[0]
                b.record()
                torch.cuda.synchronize()
                if rnd:
                    ms[kind].append(a.elapsed_time(b))
                hs[kind] = h.H
                del h
        counts = [offs[e + 1] - offs[e] for e in range(E)]
        point = {"shape": name, "E": E, "top_k": k, "n": n, "a_div": a_div, "tokens_per_call": tokens, "calls": calls,
                 "rows_per_expert_min_max": [min(counts), max(counts)]}
        for kind in kinds:
            point[kind + "_ms"] = [round(t, 3) for t in ms[kind]]
            point[kind + "_ms_median"] = round(_median(ms[kind]), 3)
        spread = max(max(ms[kind]) - min(ms[kind]) for kind in kinds)
        point["spread_ms"] = round(spread, 3)
        point["speedup"] = round(point["torch_ms_median"] / point["fused_ms_median"], 2)
        point["fused_wins_by_more_than_the_spread"] = bool(min(ms["torch"]) - max(ms["fused"]) > spread)
        point["over_dense_calls"] = round(point["fused_ms_median"] / point["dense_calls_ms_median"], 3)
        point["fused_beats_dense_calls_by_more_than_the_spread"] = bool(min(ms["dense_calls"]) - max(ms["fused"]) > spread)
        point["same_bits_as_dense_calls"] = bool(torch.equal(hs["fused"], hs["dense_calls"]))
        point["relative_difference"] = float((hs["fused"].double() - hs["torch"].double()).norm() / hs["torch"].double().norm())
        print(json.dumps(point))
        points.append(point)
        del x, rows, hs
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "points": points}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
