#!/usr/bin/env python3
"""ops.token_logprobs against the torch composition a user would write without it, on the same GPU in the same run, and the throughput of
QuantLlamaForCausalLM.score.

    fused   ops.token_logprobs(logits, targets): one launch, the fp16 logits read once from HBM
    torch   log_softmax(logits.float(), -1).gather(1, targets[:, None]) and logits.argmax(-1): an fp32 copy and an fp32 result of
            [rows, vocab] live at once
Both read one fp16 [rows, vocab] tensor and produce f32 [rows] and int64 [rows].  The grid is 512 and 2048 rows x vocab 32000 / 128256 /
151936.  Every call takes the next of several copies of the logits that together exceed 512 MiB, so that no call finds its input in the
256 MiB Infinity Cache.  The two are timed alternately in one process, ROUNDS times: CALLS calls each per round, every call between two
device events on an otherwise idle stream.  A round's value is the median of its calls; the JSON keeps every round and reports the median
of rounds, their min / max as the spread, torch / fused, and the kernel's bytes per second counted against the single fp16 read
(rows * vocab * 2 bytes over its time: the algorithm's bytes, not the traffic of its second, L2-served walk).

The second part scores 4 sequences of 2048 tokens with the four-layer Llama-2-7B-shaped random model of tools/bench_generate.py
(chunk_tokens 2048), with and without fuse_prefill(), over an fp16 and an int8 cache: tokens per second of wall time around a device
synchronise, the variants alternately, ROUNDS rounds.

    python tools/bench_score.py [--out profiles/score_bench.json] [--rows 512,2048] [--vocab 32000,128256,151936] [--no-model]
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

ROUNDS, CALLS, WARMUP = 5, 10, 3
ROTATE_BYTES = 512 << 20
SEQS, SEQLEN, LAYERS = 4, 2048, 4


def torch_score(logits, targets):
    import torch

    return torch.log_softmax(logits.float(), -1).gather(1, targets[:, None])[:, 0], logits.argmax(-1)


def point(rows, vocab, dev):
    import torch

    from bench_sample import time_calls
    from qqq_amd import ops

    g = torch.Generator(device=dev).manual_seed(vocab + rows)
    nbytes = rows * vocab * 2
    copies = max(2, -(-ROTATE_BYTES // nbytes))
    bufs = [(4.0 * torch.randn((rows, vocab), generator=g, device=dev)).half() for _ in range(copies)]
    targets = torch.randint(0, vocab, (rows,), generator=g, device=dev)
    turn = {"fused": 0, "torch": 0}

    def take(name):
        turn[name] = (turn[name] + 1) % copies
        return bufs[turn[name]]

    fns = {"fused": lambda: ops.token_logprobs(take("fused"), targets), "torch": lambda: torch_score(take("torch"), targets)}
    a, b = ops.token_logprobs(bufs[0], targets), torch_score(bufs[0], targets)
    res = {"rows": rows, "vocab": vocab, "logits_bytes": nbytes, "copies_rotated": copies,
           "max_abs_logprob_difference_to_torch_f32": float((a[0] - b[0]).abs().max()), "argmax_equal": bool(torch.equal(a[1], b[1]))}
    for f in fns.values():
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    rounds = {n: [] for n in fns}
    for _ in range(ROUNDS):
        for n, f in fns.items():
            rounds[n].append(statistics.median(time_calls(f, CALLS)))
    for n, v in rounds.items():
        res[n] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                  "rounds_us": [round(x, 2) for x in v]}
    res["torch_over_fused"] = round(res["torch"]["median_us"] / res["fused"]["median_us"], 2)
    res["torch_over_fused_range"] = [round(res["torch"]["min_us"] / res["fused"]["max_us"], 2),
                                     round(res["torch"]["max_us"] / res["fused"]["min_us"], 2)]
    res["fused_tb_per_s_of_the_single_fp16_read"] = round(nbytes / (res["fused"]["median_us"] * 1e-6) / 1e12, 3)
    return res


def model_points(dev):
    import torch

    from bench_model import VOCAB, build

    lm = build(LAYERS, dev)
    g = torch.Generator().manual_seed(0)
    seqs = [torch.randint(0, VOCAB, (SEQLEN,), generator=g).tolist() for _ in range(SEQS)]
    variants = [(kv, fused) for kv in ("fp16", "int8") for fused in (False, True)]

    def run(kv, fused):
        lm.model.fuse_prefill() if fused else lm.model.unfuse_prefill()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lp = lm.score(seqs, chunk_tokens=SEQLEN, dtype=torch.float16 if kv == "fp16" else torch.int8)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, float(torch.cat(lp).double().mean())

    values, mean_lp = {v: [] for v in variants}, {}
    for v in variants:  # warm-up: code objects, workspaces, rope tables
        mean_lp[v] = run(*v)[1]
    for _ in range(ROUNDS):
        for v in variants:
            values[v].append(SEQS * SEQLEN / run(*v)[0])
    lm.model.unfuse_prefill()
    out = []
    for (kv, fused), v in values.items():
        out.append({"kv": kv, "fuse_prefill": fused, "median_tokens_per_s": round(statistics.median(v)), "min_tokens_per_s": round(min(v)),
                    "max_tokens_per_s": round(max(v)), "rounds_tokens_per_s": [round(x) for x in v],
                    "mean_logprob": mean_lp[(kv, fused)]})
    return {"shape": f"{LAYERS} Llama-2-7B layers, per-channel W4A8, fuse_qkv(), vocab {VOCAB}, random weights", "sequences": SEQS,
            "tokens_per_sequence": SEQLEN, "chunk_tokens": SEQLEN, "variants": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.json"))
    ap.add_argument("--rows", default="512,2048")
    ap.add_argument("--vocab", default="32000,128256,151936")
    ap.add_argument("--no-model", action="store_true", help="the kernel grid alone")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_score.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        points = [point(r, v, dev) for v in map(int, args.vocab.split(",")) for r in map(int, args.rows.split(","))]
        notes = [f"rows={p['rows']} vocab={p['vocab']}: the fused op does not win ({p['torch_over_fused']}x)"
                 for p in points if p["torch_over_fused_range"][0] <= 1.0]
        out = {"tool": "tools/bench_score.py", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_round": CALLS,
               "points": points, "notes": notes or ["the fused op wins at every point, also at the unfavourable ends of both spreads"]}
        if not args.no_model:
            out["score"] = model_points(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"rows {p['rows']:5d} vocab {p['vocab']:6d}: fused {p['fused']['median_us']:9.1f} us  torch {p['torch']['median_us']:9.1f} us  "
              f"({p['torch_over_fused']}x)  {p['fused_tb_per_s_of_the_single_fp16_read']} TB/s of the fp16 read")
    for v in out.get("score", {}).get("variants", []):
        print(f"score kv {v['kv']} fuse_prefill {v['fuse_prefill']}: {v['median_tokens_per_s']} tokens/s "
              f"[{v['min_tokens_per_s']}, {v['max_tokens_per_s']}], mean log-prob {v['mean_logprob']:.4f}")


if __name__ == "__main__":
    main()
