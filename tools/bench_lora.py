#!/usr/bin/env python3
"""ops.lora_add against the torch composition a user has without it, on the same GPU, replayed from a hipGraph each.

    fused   ops.lora_add(y, xq, s1, A, B, scale, slot, part_cols): one launch for a whole projection group
    torch   index_select of A and B by the rows' slots, both cast to f32; x = xq.float() * s1; bmm(A_t, x) -> [T, P * R]; per part
            bmm(B_t[:, its columns], h[:, its rows]); times scale[slot]; added to y in f32 and rounded to fp16 in place
Shapes: Llama-2-7B's two fused groups -- q|k|v (K = 4096, N = 3 * 4096) and gate|up (K = 4096, N = 2 * 11008) -- at rank 16 and 64, T = 1, 16,
64 and 2048 rows, with one adapter for all rows and with every row on an adapter of its own (S = T slots).
Protocol (tools/bench_sample.py's, cold): the two are timed alternately in one process, ROUNDS times; a round is the median of CALLS
replays, each between two device events on an otherwise idle stream and each behind a 512 MiB fill that is not timed, so that neither
finds its adapters in a cache -- in a decoder step 100 MB of weights pass between two calls.  The JSON keeps every round, reports the
median of the rounds with their min and max, torch / fused with its range, and lists every point the op loses (its median above torch's).

    python tools/bench_lora.py [--out profiles/lora_bench.json] [--tokens 1,16,64,2048] [--ranks 16,64]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROUNDS, WARMUP = 5, 3
GROUPS = {"qkv": (4096, (0, 4096, 8192, 12288)), "gate_up": (4096, (0, 11008, 22016))}


def torch_lora(y, xq, s1, A, B, scale, slot, cols):
    import torch

    idx = slot.long()
    R = B.shape[2]
    At, Bt = A.index_select(0, idx).float(), B.index_select(0, idx).float()
    h = torch.bmm(At, (xq.float() * s1).unsqueeze(2))
    sc = scale.index_select(0, idx)[:, None]
    for p in range(len(cols) - 1):
        part = y[:, cols[p]:cols[p + 1]]
        part.copy_(part.float() + sc * torch.bmm(Bt[:, cols[p]:cols[p + 1]], h[:, p * R:(p + 1) * R]).squeeze(2))
    return y


def time_cold(fn, n, flush):
    import torch

    out = []
    for _ in range(n):
        flush.fill_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def point(group, R, T, distinct, flush, dev):
    import torch

    from bench_sample import capture
    from qqq_amd import ops

    K, cols = GROUPS[group]
    N, P, S = cols[-1], len(cols) - 1, (T if distinct else 1)
    g = torch.Generator(device=dev).manual_seed(T + R + N)
    A = torch.empty((S, P * R, K), dtype=torch.float16, device=dev).normal_(0, 0.03, generator=g)
    B = torch.empty((S, N, R), dtype=torch.float16, device=dev).normal_(0, 0.5 / R ** 0.5, generator=g)
    scale = torch.full((S,), 2.0, device=dev)
    xq = torch.randint(-127, 128, (T, K), generator=g, device=dev, dtype=torch.int8)
    s1 = torch.full((T, 1), 1.0 / (64.0 * K ** 0.5), device=dev)
    slot = (torch.randperm(T, generator=g, device=dev) if distinct else torch.zeros(T, device=dev)).int()
    y0 = torch.empty((T, N), dtype=torch.float16, device=dev).normal_(0, 2.0, generator=g)
    ys = {"fused": y0.clone(), "torch": y0.clone()}
    fns = {"fused": lambda: ops.lora_add(ys["fused"], xq, s1, A, B, scale, slot, cols),
           "torch": lambda: torch_lora(ys["torch"], xq, s1, A, B, scale, slot, cols)}
    for f in fns.values():
        f()
    diff = float((ys["fused"].float() - ys["torch"].float()).abs().max())
    calls = 20 if T <= 64 else 8
    run = {n: capture(f).replay for n, f in fns.items()}
    for f in run.values():
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    rounds = {n: [] for n in run}
    for _ in range(ROUNDS):
        for n, f in run.items():
            rounds[n].append(statistics.median(time_cold(f, calls, flush)))
    res = {"group": group, "K": K, "N": N, "P": P, "R": R, "T": T, "slots": "distinct" if distinct else "one", "max_abs_diff_after_one_call": diff}
    for n, v in rounds.items():
        res[n] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                  "rounds_us": [round(x, 2) for x in v]}
    res["torch_over_fused"] = round(res["torch"]["median_us"] / res["fused"]["median_us"], 2)
    res["torch_over_fused_range"] = [round(res["torch"]["min_us"] / res["fused"]["max_us"], 2),
                                     round(res["torch"]["max_us"] / res["fused"]["min_us"], 2)]
    res["op_loses"] = bool(res["fused"]["median_us"] > res["torch"]["median_us"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_bench.json"))
    ap.add_argument("--tokens", default="1,16,64,2048")
    ap.add_argument("--ranks", default="16,64")
    args = ap.parse_args()
    import torch

    dev = torch.device("cuda:0")
    flush = torch.empty(512 << 20, dtype=torch.int8, device=dev)
    points = []
    with torch.no_grad():
        for group in GROUPS:
            for R in map(int, args.ranks.split(",")):
                for T in map(int, args.tokens.split(",")):
                    for distinct in (False, True):
                        r = point(group, R, T, distinct, flush, dev)
                        points.append(r)
                        print(f"{group:8s} R={R:2d} T={T:4d} {r['slots']:8s} fused {r['fused']['median_us']:9.1f} us "
                              f"[{r['fused']['min_us']:.1f} - {r['fused']['max_us']:.1f}]  torch {r['torch']['median_us']:10.1f} us "
                              f"[{r['torch']['min_us']:.1f} - {r['torch']['max_us']:.1f}]  x{r['torch_over_fused']}", flush=True)
                        torch.cuda.empty_cache()
    out = {"tool": "tools/bench_lora.py", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "protocol": "hipGraph replay, cold: a 512 MiB "
           "fill in front of every timed replay; a round is the median of its calls, a point the median of its rounds with their min and max",
           "points": points, "op_loses": [{k: p[k] for k in ("group", "R", "T", "slots")} for p in points if p["op_loses"]]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("lost points:", out["op_loses"])


if __name__ == "__main__":
    main()
