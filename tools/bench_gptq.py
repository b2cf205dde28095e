#!/usr/bin/env python3
"""gptq_quantize with the fused column sweep (one HIP launch per 128-column block) against the same flow with the sweep composed from
torch calls (fused=False: a handful of launches per weight column, what the reference does), on the same GPU, at Llama-2-7B's linear
shapes, per-channel and g128.  Wall time per call with a synchronise on both sides, and the split of the GPU time into the scale search,
the sweep, the trailing GEMM and the Cholesky chain from events around those sections.

    python tools/bench_gptq.py [--rounds 5] [--out profiles/gptq_bench.json] [--small] [--act-order]

--act-order times gptq_quantize_ordered (act-order, and static groups when grouped) instead: fused (ops.gptq_block_cols) against its own
fused=False, and against plain gptq_quantize fused, with the split also showing the one-launch group scales and the permutation gathers;
the default --out is then profiles/gptq_order_bench.json.

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
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "gptq_order_bench.json" if args.act_order else "gptq_bench.json")
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
        for gs in () if args.act_order else (-1, 128):
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


if __name__ == "__main__":
    main()
