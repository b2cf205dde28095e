#!/usr/bin/env python3
"""The smoothing search's fake-quantisation as one HIP launch (ops.fake_quant_rows) against the same arithmetic composed from torch calls
(smooth.fake_quant_torch: about fourteen launches, what the reference runs per operand and candidate), on the same GPU, at Llama-2-7B's
shapes with the reference's calibration batch (8 x 2048 tokens):

    activations (8 bits per token, x / s)   16384 x 4096, 16384 x 11008
    weights (4 bits, W * s)                 12288 x 4096 (q|k|v), 22016 x 4096 (gate|up), 4096 x 11008 (down); per-channel and g128

and the whole os+ search (migration_scale) of each of the four module kinds at those sizes, fused against composed, with the candidate
count, the chosen index and its loss from both.

    python tools/bench_smooth.py [--rounds 5] [--iters 10] [--search-rounds 3] [--out profiles/smooth_bench.json] [--small]

Per op: `iters` calls between two events, fused and composed alternating, the median of `rounds`.  Per search: wall time with a
synchronise on both sides, the median of `search-rounds`.  Writes the JSON and prints one line per point.  Nothing asserts a time.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--search-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bench.json"))
    ap.add_argument("--small", action="store_true", help="a sixteenth of the tokens and an eighth of the widths: a rehearsal, not a measurement")
    ap.add_argument("--skip-search", action="store_true")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_smooth.py needs a GPU: there is no CPU path")
    from qqq_amd.quant import ops
    from qqq_amd.quant.smooth import attention_extra, fake_quant_torch, migration_scale
    from types import SimpleNamespace

    dev = torch.device("cuda:0")
    B, N, H, I, heads = (2, 512, 512, 1376, 4) if args.small else (8, 2048, 4096, 11008, 32)
    gen = torch.Generator(device="cpu").manual_seed(0)

    def activation(K):
        x = torch.randn((B, N, K), generator=gen)
        for j, f in ((7, 12.0), (K // 3, -9.0), (K - 9, 6.0)):  # outlier channels of both signs
            x[:, :, j] *= f
        return x.half().to(dev)

    def weight(rows, K):
        return (torch.randn((rows, K), generator=gen) * K ** -0.5).half().to(dev)

    def col_scale(K):
        s = torch.ones(K)
        s[torch.randperm(K, generator=gen)[: K // 16]] = torch.rand(K // 16, generator=gen) * 6 + 1
        return s.half().to(dev)

    def time_pair(x, c, bits, group, divide):
        out = torch.empty_like(x)
        calls = {"fused": lambda: ops.fake_quant_rows(x, c, bits, group, divide, out=out), "composed": lambda: fake_quant_torch(x, c, bits, group, divide)}
        same = torch.equal(calls["fused"](), calls["composed"]())  # also the warm-up
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, f in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    f()
                b.record()
                torch.cuda.synchronize()
                times[k].append(a.elapsed_time(b) / args.iters)
        med = {k: statistics.median(v) for k, v in times.items()}
        nbytes = 2 * x.numel() * 2  # one read, one write
        return {"fused_ms": round(med["fused"], 4), "composed_ms": round(med["composed"], 4), "ratio": round(med["composed"] / med["fused"], 2),
                "fused_GBps": round(nbytes / med["fused"] / 1e6, 1), "fused_ms_all": [round(t, 4) for t in times["fused"]],
                "composed_ms_all": [round(t, 4) for t in times["composed"]], "same_bits": same}

    report = {"device": torch.cuda.get_device_name(0), "small": args.small, "rounds": args.rounds, "iters": args.iters, "ops": [], "searches": []}
    acts = {K: activation(K) for K in (H, I)}
    for K, x in acts.items():
        r = dict(operand="activation", rows=B * N, cols=K, bits=8, group=0, **time_pair(x.reshape(B * N, K), col_scale(K), 8, 0, True))
        report["ops"].append(r)
        print(json.dumps(r), flush=True)
    weights = {"qkv": weight(3 * H, H), "up_and_gate": weight(2 * I, H), "down_proj": weight(H, I)}
    for kind, w in weights.items():
        for group in (0, 128):
            r = dict(operand="weight " + kind, rows=w.shape[0], cols=w.shape[1], bits=4, group=group, **time_pair(w, col_scale(w.shape[1]), 4, group, False))
            report["ops"].append(r)
            print(json.dumps(r), flush=True)
    if not args.skip_search:
        weights["o_proj"] = weight(H, H)
        cfg = SimpleNamespace(num_attention_heads=heads, num_key_value_heads=heads, hidden_size=H, rope_theta=10000.0)
        extra = attention_extra(cfg, N, dev)
        for kind in ("qkv", "o_proj", "up_and_gate", "down_proj"):
            x, w = acts[I if kind == "down_proj" else H], weights[kind]
            for group_size in (-1, 128):
                times, traces, scales = {"fused": [], "composed": []}, {}, {}
                for rnd in range(args.search_rounds + 1):  # round 0 is the warm-up
                    for k in times:
                        tr = {}
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        scales[k] = migration_scale(x, w, kind, group_size, "os+", extra if kind == "qkv" else None, fused=k == "fused", trace=tr)
                        torch.cuda.synchronize()
                        if rnd:
                            times[k].append(time.perf_counter() - t0)
                        traces[k] = tr
                med = {k: statistics.median(v) for k, v in times.items()}
                r = dict(kind=kind, tokens=B * N, weight=list(w.shape), group_size=group_size, candidates=len(traces["fused"]["ranges"]),
                         fused_s=round(med["fused"], 3), composed_s=round(med["composed"], 3), ratio=round(med["composed"] / med["fused"], 3),
                         fused_s_all=[round(t, 3) for t in times["fused"]], composed_s_all=[round(t, 3) for t in times["composed"]],
                         best={k: traces[k]["best"] for k in traces}, best_loss={k: traces[k]["losses"][traces[k]["best"]] for k in traces},
                         first_loss={k: traces[k]["losses"][0] for k in traces}, same_scale=torch.equal(scales["fused"], scales["composed"]),
                         same_losses=traces["fused"]["losses"] == traces["composed"]["losses"])
                report["searches"].append(r)
                print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
