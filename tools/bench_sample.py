#!/usr/bin/env python3
"""ops.sample_tokens against a torch composition of the same semantics, on the same GPU.

    fused   ops.sample_tokens(logits, T, k, p, u): one launch
    torch   logits.float() / T; torch.topk's k-th value as a threshold (ties kept); softmax; a full sort for top-p, cumsum, the cut as a
            threshold on the probability (ties together), renormalise; cumsum in token order and the first index above u * total.  The
            parameters are the same for every row, which is the cheap case for torch (one k for torch.topk, no per-row gather).
Both read one fp16 [rows, vocab] tensor and write int64 [rows].  The two are timed alternately in one process, ROUNDS times: CALLS calls each
per round, every call between two device events on an otherwise idle stream (eager), then the same replayed from a hipGraph each (graph).
A round's value is the median of its calls; the JSON keeps every round and reports the median of rounds, their min / max as the spread, and
torch / fused.  Logits are fp16(4 N(0, 1)), T = 0.8, k = 50, p = 0.9; `--mode` picks which cuts are on.

    python tools/bench_sample.py [--out profiles/sample_bench.json] [--rows 1,16,64] [--vocab 32000,128256,151936]

With --penalties the tool times ops.penalize_logits alone instead, against a torch composition of the same semantics, by the same protocol:

    fused   ops.penalize_logits(logits, ids, pos, seen, n_prompt, repetition, presence, frequency, workspace): one launch
    torch   per logits row of a row: the history and the drafts in front of it as one index tensor; the output counts by a scatter_add
            into [rows, vocab] (a bincount per row); gather of the counts and of the logits at the history's tokens; where() for the
            repetition rule and for c > 0; scatter of the results back (equal tokens write equal values)
Both rewrite fp16 [rows * G, vocab] in place.  Points: every vocab and rows above x histories of 128, 2048 and 16384 tokens x G = 1 and 5 x
the all-distinct and the all-one-token history, half of it prompt; penalties 1.3, 0.5, 0.25.  Written: the op's time per point, torch's,
torch / fused with the range over the rounds, and the share of logit bits the two agree on after one call.

    python tools/bench_sample.py --penalties [--out profiles/penalty_bench.json] [--rows 1,16,64] [--vocab 32000,128256,151936]

With --logprobs it times ops.topk_logprobs alone, against a torch composition of the same semantics, by the same protocol:

    fused   ops.topk_logprobs(logits, tokens, k): one launch
    torch   log_softmax(logits.float()); gather at the tokens; a rank count (logits > the token's logit, summed); torch.topk for k > 0
Points: every vocab and rows above x k = 0, 5 and 20.  Written: both times per point, torch / fused with the range over the rounds, the
share of rows whose top-k ids agree and the largest difference of a log-probability.

    python tools/bench_sample.py --logprobs [--out profiles/logprobs_bench.json] [--rows 1,16,64] [--vocab 32000,128256,151936]

With --fsm it times ops.fsm_mask and ops.fsm_advance (guided decoding) alone, each against a torch composition, by the same protocol:

    fused   ops.fsm_mask(logits, state, tables): one launch;  ops.fsm_advance(out, n_out, n_fsm, state, tables, ...): one launch
    torch   the automaton as dense tables: a bool [S, vocab] indexed by the rows' states and masked_fill_ of its complement; an int32
            [S, vocab] of next states (-2: no edge) gathered at (state, the row's last token).  The dense tables take S * vocab * 5 bytes, which
            is what rules them out beyond small automata; retiring a row and the eos rule are left out of the torch side.
Points: every vocab and rows above x 1, 64 and 20000 allowed tokens per state, 16 states that share one token set (so that every call of
the advance finds an edge) with random targets.  Every call of either advance is preceded by n_fsm.fill_(n_out - 1), or the op would find
nothing new from the second call on; both sides carry that launch, and each call advances over one token.  Written: both times per point and op, torch / fused with the range over the
rounds, and whether the two agree after one call.

    python tools/bench_sample.py --fsm [--out profiles/fsm_bench.json] [--rows 1,16,64] [--vocab 32000,128256,151936]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, CALLS, WARMUP = 5, 20, 5
MODES = {"sample": (0.8, 0, 1.0), "top_k": (0.8, 50, 1.0), "top_p": (0.8, 0, 0.9), "top_k_top_p": (0.8, 50, 0.9)}


def torch_sample(logits, T, k, p, u):
    import torch

    x = logits.float() / T
    if k > 0:
        kth = torch.topk(x, k, dim=-1).values[:, -1:]
        x = x.masked_fill(x < kth, float("-inf"))
    probs = torch.softmax(x, dim=-1)
    if p < 1.0:
        srt, _ = torch.sort(probs, dim=-1)  # ascending: the mass of everything no more probable
        cum = srt.cumsum(dim=-1)
        first = (cum > (1.0 - p)).int().argmax(dim=-1, keepdim=True)  # the least probable value that stays
        probs = probs.masked_fill(probs < srt.gather(1, first), 0.0)
    c = probs.cumsum(dim=-1)
    return (c > u[:, None] * c[:, -1:]).int().argmax(dim=-1)


def time_calls(fn, n):
    import torch

    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def capture(fn):
    import torch

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def point(rows, vocab, mode, dev):
    import torch

    from qqq_amd import ops

    T, k, p = MODES[mode]
    g = torch.Generator(device=dev).manual_seed(vocab + rows)
    logits = (4.0 * torch.randn((rows, vocab), generator=g, device=dev)).half()
    u = torch.rand(rows, generator=g, device=dev)
    Tt, kt, pt = (torch.full((rows,), v, dtype=dt, device=dev) for v, dt in ((T, torch.float32), (k, torch.int32), (p, torch.float32)))
    fns = {"fused": lambda: ops.sample_tokens(logits, Tt, kt, pt, u), "torch": lambda: torch_sample(logits, T, k, p, u)}
    same = float((fns["fused"]() == fns["torch"]()).float().mean())  # f32 against exact sums: a row may differ at a cut or an edge
    res = {"rows": rows, "vocab": vocab, "mode": mode, "rows_equal_fraction": same}
    for how in ("eager", "graph"):
        run = fns if how == "eager" else {n: capture(f).replay for n, f in fns.items()}
        for f in run.values():
            for _ in range(WARMUP):
                f()
        torch.cuda.synchronize()
        rounds = {n: [] for n in run}
        for _ in range(ROUNDS):
            for n, f in run.items():
                rounds[n].append(statistics.median(time_calls(f, CALLS)))
        r = {}
        for n, v in rounds.items():
            r[n] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                    "rounds_us": [round(x, 2) for x in v]}
        r["torch_over_fused"] = round(r["torch"]["median_us"] / r["fused"]["median_us"], 2)
        r["torch_over_fused_range"] = [round(r["torch"]["min_us"] / r["fused"]["max_us"], 2), round(r["torch"]["max_us"] / r["fused"]["min_us"], 2)]
        res[how] = r
    return res


PENALTIES, HISTORIES, GROUPS, CONTENTS = (1.3, 0.5, 0.25), (128, 2048, 16384), (1, 5), ("distinct", "one_token")


def torch_penalize(logits, ids, pos, seen, n_prompt, rep, pres, freq):
    """The semantics of include/qqq_amd_penalty.h for rows that share one position and hold valid tokens only (what the points are)."""
    import torch

    rows, group = ids.shape
    vocab, n = logits.shape[1], seen.shape[1]  # the history fills `seen`: p + 1 = seen_stride
    seen[:, n - 1] = ids[:, 0]
    hist = seen.long()
    for j in range(group):
        seq = torch.cat([hist, ids[:, 1:j + 1]], dim=1)
        is_out = (torch.arange(n + j, device=seq.device)[None] >= n_prompt[:, None]).float()
        counts = torch.zeros((rows, vocab), device=seq.device).scatter_add_(1, seq, is_out)
        c = counts.gather(1, seq)
        row = logits[j::group]
        x = row.gather(1, seq).float()
        x = torch.where(x > 0, x / rep[:, None], x * rep[:, None])
        x = torch.where(c > 0, x - freq[:, None] * c - pres[:, None], x)
        row.scatter_(1, seq, x.half())
    return logits


def penalty_point(rows, vocab, n, group, content, dev):
    import torch

    from qqq_amd import ops

    g = torch.Generator(device=dev).manual_seed(vocab + rows + n + group)
    fresh = (4.0 * torch.randn((rows * group, vocab), generator=g, device=dev)).half()
    if content == "distinct":
        tokens = torch.stack([torch.randperm(vocab, generator=g, device=dev)[:n + group - 1] for _ in range(rows)])
    else:
        tokens = torch.randint(0, vocab, (rows, 1), generator=g, device=dev).expand(rows, n + group - 1).contiguous()
    seen = tokens[:, :n].int().contiguous()
    ids = tokens[:, n - 1:].contiguous()
    pos = (n - 1 + torch.arange(group, device=dev))[None].expand(rows, group).contiguous()
    n_prompt = torch.full((rows,), n // 2, dtype=torch.int32, device=dev)
    rep, pres, freq = (torch.full((rows,), v, dtype=torch.float32, device=dev) for v in PENALTIES)
    ws = torch.zeros(rows * vocab, dtype=torch.int32, device=dev)
    bufs = {"fused": fresh.clone(), "torch": fresh.clone()}
    fns = {"fused": lambda: ops.penalize_logits(bufs["fused"], ids, pos, seen, n_prompt, rep, pres, freq, ws),
           "torch": lambda: torch_penalize(bufs["torch"], ids, pos, seen, n_prompt, rep, pres, freq)}
    same = float((fns["fused"]().view(torch.int16) == fns["torch"]().view(torch.int16)).float().mean())
    res = {"rows": rows, "vocab": vocab, "history": n, "group": group, "content": content, "bits_equal_fraction": same}
    for how in ("eager", "graph"):  # the values drift as the penalties pile up call after call; the work does not depend on them
        run = fns if how == "eager" else {name: capture(f).replay for name, f in fns.items()}
        for f in run.values():
            for _ in range(WARMUP):
                f()
        torch.cuda.synchronize()
        rounds = {name: [] for name in run}
        for _ in range(ROUNDS):
            for name, f in run.items():
                rounds[name].append(statistics.median(time_calls(f, CALLS)))
        r = {}
        for name, v in rounds.items():
            r[name] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                       "rounds_us": [round(x, 2) for x in v]}
        r["torch_over_fused"] = round(r["torch"]["median_us"] / r["fused"]["median_us"], 2)
        r["torch_over_fused_range"] = [round(r["torch"]["min_us"] / r["fused"]["max_us"], 2), round(r["torch"]["max_us"] / r["fused"]["min_us"], 2)]
        res[how] = r
    assert int(torch.count_nonzero(ws)) == 0
    return res


def penalty_main(args, dev):
    import torch

    points = [penalty_point(r, v, n, g, c, dev) for v in map(int, args.vocab.split(",")) for r in map(int, args.rows.split(","))
              for n in HISTORIES for g in GROUPS for c in CONTENTS]
    notes = [f"rows={p['rows']} vocab={p['vocab']} history={p['history']} G={p['group']} {p['content']} {how}: the op does not win "
             f"({p[how]['torch_over_fused']}x)" for p in points for how in ("eager", "graph") if p[how]["torch_over_fused_range"][0] <= 1.0]
    out = {"tool": "tools/bench_sample.py --penalties", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_round": CALLS,
           "penalties": dict(zip(("repetition", "presence", "frequency"), PENALTIES)), "points": points,
           "notes": notes or ["the op wins at every point, also at the unfavourable ends of both spreads"]}
    path = args.out or os.path.join(ROOT, "profiles", "penalty_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"rows {p['rows']:3d} vocab {p['vocab']:6d} history {p['history']:5d} G {p['group']} {p['content']:9s}: " + "  ".join(
            f"{how} fused {p[how]['fused']['median_us']:8.1f} us torch {p[how]['torch']['median_us']:8.1f} us ({p[how]['torch_over_fused']}x)"
            for how in ("eager", "graph")))


LOGPROB_KS = (0, 5, 20)


def torch_logprobs(logits, tokens, k):
    import torch

    ls = torch.log_softmax(logits.float(), dim=-1)
    at = logits.gather(1, tokens[:, None])
    out = (ls.gather(1, tokens[:, None])[:, 0], 1 + (logits > at).sum(dim=-1))
    return out + tuple(torch.topk(ls, k, dim=-1)) if k else out


def logprobs_point(rows, vocab, k, dev):
    import torch

    from qqq_amd import ops

    g = torch.Generator(device=dev).manual_seed(vocab + rows + k)
    logits = (4.0 * torch.randn((rows, vocab), generator=g, device=dev)).half()
    tokens = torch.randint(0, vocab, (rows,), generator=g, device=dev)
    fns = {"fused": lambda: ops.topk_logprobs(logits, tokens, k), "torch": lambda: torch_logprobs(logits, tokens, k)}
    a, b = fns["fused"](), fns["torch"]()
    res = {"rows": rows, "vocab": vocab, "k": k, "max_logprob_difference": float((a[0] - b[0]).abs().max()),
           "ranks_equal_fraction": float((a[1] == b[1]).float().mean())}
    if k:  # torch.topk breaks ties its own way: fp16 logits repeat
        res["top_ids_equal_fraction"] = float((a[2] == b[3]).all(dim=-1).float().mean())
    for how in ("eager", "graph"):
        run = fns if how == "eager" else {name: capture(f).replay for name, f in fns.items()}
        for f in run.values():
            for _ in range(WARMUP):
                f()
        torch.cuda.synchronize()
        rounds = {name: [] for name in run}
        for _ in range(ROUNDS):
            for name, f in run.items():
                rounds[name].append(statistics.median(time_calls(f, CALLS)))
        r = {}
        for name, v in rounds.items():
            r[name] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                       "rounds_us": [round(x, 2) for x in v]}
        r["torch_over_fused"] = round(r["torch"]["median_us"] / r["fused"]["median_us"], 2)
        r["torch_over_fused_range"] = [round(r["torch"]["min_us"] / r["fused"]["max_us"], 2), round(r["torch"]["max_us"] / r["fused"]["min_us"], 2)]
        res[how] = r
    return res


def logprobs_main(args, dev):
    import torch

    points = [logprobs_point(r, v, k, dev) for v in map(int, args.vocab.split(",")) for r in map(int, args.rows.split(",")) for k in LOGPROB_KS]
    notes = [f"rows={p['rows']} vocab={p['vocab']} k={p['k']} {how}: the op does not win ({p[how]['torch_over_fused']}x)"
             for p in points for how in ("eager", "graph") if p[how]["torch_over_fused_range"][0] <= 1.0]
    out = {"tool": "tools/bench_sample.py --logprobs", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_round": CALLS,
           "points": points, "notes": notes or ["the op wins at every point, also at the unfavourable ends of both spreads"]}
    path = args.out or os.path.join(ROOT, "profiles", "logprobs_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"rows {p['rows']:3d} vocab {p['vocab']:6d} k {p['k']:2d}: " + "  ".join(
            f"{how} fused {p[how]['fused']['median_us']:8.1f} us torch {p[how]['torch']['median_us']:8.1f} us ({p[how]['torch_over_fused']}x)"
            for how in ("eager", "graph")))


FSM_ALLOWED, FSM_STATES = (1, 64, 20000), 16


def rotate(fns):
    """the protocol of every point: eager, then replayed from a graph each; ROUNDS rounds of the median of CALLS calls, alternately"""
    import torch

    res = {}
    for how in ("eager", "graph"):
        run = fns if how == "eager" else {name: capture(f).replay for name, f in fns.items()}
        for f in run.values():
            for _ in range(WARMUP):
                f()
        torch.cuda.synchronize()
        rounds = {name: [] for name in run}
        for _ in range(ROUNDS):
            for name, f in run.items():
                rounds[name].append(statistics.median(time_calls(f, CALLS)))
        r = {}
        for name, v in rounds.items():
            r[name] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                       "rounds_us": [round(x, 2) for x in v]}
        r["torch_over_fused"] = round(r["torch"]["median_us"] / r["fused"]["median_us"], 2)
        r["torch_over_fused_range"] = [round(r["torch"]["min_us"] / r["fused"]["max_us"], 2), round(r["torch"]["max_us"] / r["fused"]["min_us"], 2)]
        res[how] = r
    return res


def fsm_point(rows, vocab, allowed, dev):
    import numpy as np
    import torch

    from qqq_amd import TokenFSM, ops

    rng = np.random.default_rng(vocab + rows + allowed)
    S = FSM_STATES
    toks = np.sort(rng.choice(vocab, size=allowed, replace=False))
    fsm = TokenFSM(np.arange(S + 1) * allowed, np.tile(toks, S), rng.integers(0, S, size=S * allowed), np.zeros(S, np.int32), 0, vocab)
    tables = fsm.tensors(dev)
    dense_ok = torch.zeros((S, vocab), dtype=torch.bool, device=dev)
    dense_ok[:, torch.from_numpy(toks).to(dev)] = True
    dense_next = torch.full((S, vocab), -2, dtype=torch.int32, device=dev)
    dense_next[:, torch.from_numpy(toks).to(dev)] = tables[2].view(S, allowed)
    g = torch.Generator(device=dev).manual_seed(vocab + rows + allowed)
    fresh = (4.0 * torch.randn((rows, vocab), generator=g, device=dev)).half()
    state0 = torch.randint(0, S, (rows,), generator=g, device=dev, dtype=torch.int32)
    out = torch.from_numpy(rng.choice(toks, size=(rows, 4))).to(dev)
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    n_out, n_fsm, remaining = torch.full((rows,), 3, **i32), torch.zeros(rows, **i32), torch.ones(rows, **i32)
    ids, pos, slots = torch.zeros(rows, **i64), torch.zeros(rows, **i64), torch.zeros(rows, **i64)
    bufs = {"fused": fresh.clone(), "torch": fresh.clone()}
    states = {"fused": state0.clone(), "torch": state0.clone()}

    def torch_mask():
        return bufs["torch"].masked_fill_(~dense_ok[state0.long()], float("-inf"))

    def fused_advance():
        n_fsm.fill_(2)
        ops.fsm_advance(out, n_out, n_fsm, states["fused"], tables, ids, pos, slots, remaining)

    def torch_advance():
        n_fsm.fill_(2)
        states["torch"].copy_(dense_next[states["torch"].long(), out[:, 2]])

    mask = {"fused": lambda: ops.fsm_mask(bufs["fused"], state0, tables), "torch": torch_mask}
    same = bool((mask["fused"]().view(torch.int16) == mask["torch"]().view(torch.int16)).all())
    fused_advance()
    torch_advance()
    same_state = bool((states["fused"] == states["torch"]).all()) and int(remaining.min()) == 1
    res = {"rows": rows, "vocab": vocab, "allowed": allowed, "states": S, "mask_bits_equal": same, "advance_states_equal": same_state,
           "mask": rotate(mask), "advance": rotate({"fused": fused_advance, "torch": torch_advance})}
    assert bool((states["fused"] == states["torch"]).all())
    return res


def fsm_main(args, dev):
    import torch

    points = [fsm_point(r, v, a, dev) for v in map(int, args.vocab.split(",")) for r in map(int, args.rows.split(",")) for a in FSM_ALLOWED]
    notes = [f"{op} rows={p['rows']} vocab={p['vocab']} allowed={p['allowed']} {how}: the op does not win ({p[op][how]['torch_over_fused']}x)"
             for p in points for op in ("mask", "advance") for how in ("eager", "graph") if p[op][how]["torch_over_fused_range"][0] <= 1.0]
    out = {"tool": "tools/bench_sample.py --fsm", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_round": CALLS,
           "points": points, "notes": notes or ["both ops win at every point, also at the unfavourable ends of both spreads"]}
    path = args.out or os.path.join(ROOT, "profiles", "fsm_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"rows {p['rows']:3d} vocab {p['vocab']:6d} allowed {p['allowed']:5d}: " + "  ".join(
            f"{op} {how} fused {p[op][how]['fused']['median_us']:7.1f} us torch {p[op][how]['torch']['median_us']:7.1f} us ({p[op][how]['torch_over_fused']}x)"
            for op in ("mask", "advance") for how in ("eager", "graph")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/sample_bench.json, profiles/penalty_bench.json with --penalties, profiles/logprobs_bench.json with --logprobs")
    ap.add_argument("--penalties", action="store_true", help="time ops.penalize_logits against a torch composition instead")
    ap.add_argument("--logprobs", action="store_true", help="time ops.topk_logprobs against a torch composition instead")
    ap.add_argument("--fsm", action="store_true", help="time ops.fsm_mask and ops.fsm_advance against torch compositions instead (profiles/fsm_bench.json)")
    ap.add_argument("--rows", default="1,16,64")
    ap.add_argument("--vocab", default="32000,128256,151936")
    ap.add_argument("--modes", default="sample,top_k_top_p")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_sample.py needs a GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    if args.penalties:
        return penalty_main(args, dev)
    if args.logprobs:
        return logprobs_main(args, dev)
    if args.fsm:
        return fsm_main(args, dev)
    args.out = args.out or os.path.join(ROOT, "profiles", "sample_bench.json")
    points = [point(r, v, m, dev) for m in args.modes.split(",") for v in map(int, args.vocab.split(",")) for r in map(int, args.rows.split(","))]
    notes = [f"{p['mode']} rows={p['rows']} vocab={p['vocab']} {how}: the fused op does not win ({p[how]['torch_over_fused']}x)"
             for p in points for how in ("eager", "graph") if p[how]["torch_over_fused_range"][0] <= 1.0]
    out = {"tool": "tools/bench_sample.py", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_round": CALLS,
           "modes": {m: dict(zip(("temperature", "top_k", "top_p"), MODES[m])) for m in args.modes.split(",")}, "points": points,
           "notes": notes or ["the fused op wins at every point, also at the unfavourable ends of both spreads"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in points:
        print(f"{p['mode']:12s} rows {p['rows']:3d} vocab {p['vocab']:6d}: " + "  ".join(
            f"{how} fused {p[how]['fused']['median_us']:8.1f} us torch {p[how]['torch']['median_us']:8.1f} us ({p[how]['torch_over_fused']}x)"
            for how in ("eager", "graph")))


if __name__ == "__main__":
    main()
