#!/usr/bin/env python3
"""ops.hadamard_rows against the reference's way of applying the same matrices, on the same GPU, at Llama-2-7B's weight shapes in fp16:

    n = 4096 (the residual rotation)   the reference: (W.double() @ Q).to(fp16), Q = diag(s) H / 64 in f64 -- an O(n^2) product per row.
                                       4096 x 11008 is down_proj, turned on its OUTPUT side: Q^T W there, and here the op on
                                       W.t().contiguous() transposed back (the two copies are timed with the op: "op_path_ms")
    n = 128  (the per-head step)       the reference: an f32 butterfly in a CUDA package that is not available here; its stand-in is
                                       the dense product of every block with H_128: (W.float().view(rows, -1, 128) @ H * scale).half()

Five rounds; in each round every variant times its calls back to back between two events after a warm-up call (200 of the op, 5 of
the f64 product, 50 of the per-head product), the variants alternating.
Reported per point: the per-call times, medians, the op's bytes (one read and one write of the matrix) over its median against the HBM
rates of the MI355X (8.0 TB/s specified, 6.29 TB/s measured for a float4 copy), whether both matrices fit the 256 MB Infinity Cache (a
rate above the HBM figure is then the cache's), whether the results are the same bits, and whether the op beats the dense product by
more than the spread.

    python tools/bench_rotate.py [--rounds 5] [--out profiles/rotate_bench.json] [--small]

--k: ops.hadamard_rows_k at the hidden sizes K * 2^p (n = 896 = 28 * 32, 1536 = 12 * 128, 3584 = 28 * 128, 5120 = 40 * 128), the residual
rotation of 4096 x n, 11008 x n, and 32000 x n (151936 x n at the Qwen2 sizes 896, 1536, 3584) matrices in fp16, by the same protocol,
into profiles/rotate_k_bench.json.  Against the dense line (W.double() @ Q).half() with Q = hadamard_matrix_k(...) on the same GPU (same
bits checked; the 151936-row products run in slices of 16384 rows), and against ops.hadamard_rows on the same rows at the nearest
power of two (the same number of elements where the shapes allow it): what the K-mix costs on top of the butterflies.

    python tools/bench_rotate.py --k [--rounds 5] [--out profiles/rotate_k_bench.json] [--small]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008), (32000, 4096)]  # q/k/v/o, gate/up, down, embeddings / lm_head of Llama-2-7B
HBM_SPEC, HBM_MEASURED, L3_BYTES = 8.0e12, 6.29e12, 256 * 2**20


def timed(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def median(v):
    return sorted(v)[len(v) // 2]


K_SIZES = [(896, 151936), (1536, 151936), (3584, 151936), (5120, 32000)]  # n and the vocabulary rows that go with it


def nearest_pow2(n):
    lo = 1 << (n.bit_length() - 1)
    return lo if n - lo <= 2 * lo - n else 2 * lo


def main_k(args, torch):
    from qqq_amd.quant import hadamard_factor, hadamard_matrix_k, hadamard_signs, hadamard_table, ops

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    points = []
    for n, vocab in ([(96, 512)] if args.small else K_SIZES):
        K, m = hadamard_factor(n)
        table = hadamard_table(K)
        signs = hadamard_signs(n, torch.Generator().manual_seed(n))
        td, sd = table.to(dev), signs.to(dev)
        Q = hadamard_matrix_k(signs, table, m).to(dev)
        p2 = nearest_pow2(n)
        s2 = hadamard_signs(p2, torch.Generator().manual_seed(p2)).to(dev)
        for rows in ((64, vocab) if args.small else (4096, 11008, vocab)):
            W = (torch.randn((rows, n), generator=g, device=dev) * 0.02).half()
            W2 = (torch.randn((rows, p2), generator=g, device=dev) * 0.02).half()  # the power-of-two op on as many rows

            def dense():
                if rows <= 16384:
                    return (W.double() @ Q).half()
                return torch.cat([(W[i:i + 16384].double() @ Q).half() for i in range(0, rows, 16384)])

            variants = {"op": lambda: ops.hadamard_rows_k(W, m, td, sign=sd), "dense": dense, "pow2": lambda: ops.hadamard_rows(W2, p2, sign=s2)}
            outs = {k: f() for k, f in variants.items()}
            torch.cuda.synchronize()
            point = {"rows": rows, "n": n, "K": K, "m": m, "pow2_n": p2, "same_bits_as_dense": bool(torch.equal(outs["op"], outs["dense"])),
                     "max_abs_difference": float((outs["op"].double() - outs["dense"].double()).abs().max())}
            del outs
            iters = {"op": 200 if rows <= 32000 else 50, "dense": 5 if rows <= 32000 else 2, "pow2": 200 if rows <= 32000 else 50}
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, f in variants.items():  # alternating
                    f()
                    times[k].append(timed(torch, f, iters[k]))
            for k, v in times.items():
                point[k + "_ms"] = [round(t, 4) for t in v]
                point[k + "_ms_median"] = round(median(v), 4)
            nbytes = 2 * rows * n * 2  # one read and one write of the fp16 matrix
            rate = nbytes / (point["op_ms_median"] * 1e-3)
            point["op_bytes"] = nbytes
            point["op_tb_per_s"] = round(rate / 1e12, 3)
            point["op_fraction_of_hbm_spec_8.0"] = round(rate / HBM_SPEC, 3)
            point["pow2_tb_per_s"] = round(2 * rows * p2 * 2 / (point["pow2_ms_median"] * 1e-3) / 1e12, 3)
            point["fits_infinity_cache"] = bool(nbytes <= L3_BYTES)
            spread = max(max(times[k]) - min(times[k]) for k in ("op", "dense"))
            point["spread_ms"] = round(spread, 4)
            point["dense_over_op"] = round(point["dense_ms_median"] / point["op_ms_median"], 1)
            point["op_wins_by_more_than_the_spread"] = bool(min(times["dense"]) - max(times["op"]) > spread)
            # per element, against the power-of-two op: the cost of the K-mix (and of log2 m instead of log2 n stages)
            point["op_ns_per_kelement_over_pow2"] = round((point["op_ms_median"] / n) / (point["pow2_ms_median"] / p2), 2)
            print(json.dumps(point))
            points.append(point)
            del variants, W, W2
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "dtype": "float16", "points": points}, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="profiles/rotate_bench.json, or profiles/rotate_k_bench.json with --k")
    ap.add_argument("--small", action="store_true", help="one 512 x 256 point per n: the plumbing alone")
    ap.add_argument("--k", action="store_true", help="ops.hadamard_rows_k at the hidden sizes K * 2^p")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "rotate_k_bench.json" if args.k else "rotate_bench.json")
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_rotate.py needs a GPU")
    if args.k:
        return main_k(args, torch)
    from qqq_amd.quant import hadamard_matrix, hadamard_signs, ops

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    points = []
    for rows, cols in ([(512, 256)] if args.small else SHAPES):
        W = (torch.randn((rows, cols), generator=g, device=dev) * 0.02).half()
        for n in ((256, 128) if args.small else (4096, 128)):
            transposed = cols % n != 0  # the output-side use: the op runs on W^T
            signs = hadamard_signs(n, torch.Generator().manual_seed(n))
            sd = signs.to(dev) if n != 128 else None
            variants = {}
            if n != 128:
                assert (rows if transposed else cols) == n, "the dense product by Q needs the rotated side to be n wide"
                Q = hadamard_matrix(signs).to(dev)
                if transposed:
                    Wt = W.t().contiguous()
                    variants["op"] = lambda: ops.hadamard_rows(Wt, n, sign=sd)
                    variants["op_path"] = lambda: ops.hadamard_rows(W.t().contiguous(), n, sign=sd).t().contiguous()
                    variants["dense"] = lambda: (Q.T @ W.double()).half()
                else:
                    variants["op"] = lambda: ops.hadamard_rows(W, n, sign=sd)
                    variants["dense"] = lambda: (W.double() @ Q).half()
            else:
                H = (hadamard_matrix(torch.ones(n, dtype=torch.int8)) * float(n) ** 0.5).round().float().to(dev)  # the +-1 matrix
                scale = 1.0 / float(n) ** 0.5
                variants["op"] = lambda: ops.hadamard_rows(W, n)
                variants["dense"] = lambda: ((W.float().view(rows, cols // n, n) @ H) * scale).half().view(rows, cols)
            outs = {k: f() for k, f in variants.items()}  # warm-up of every variant at this shape, and the results to compare
            torch.cuda.synchronize()
            ref = outs.get("op_path", outs["op"])
            point = {"rows": rows, "cols": cols, "n": n, "use": "output side (op on the transpose)" if transposed else "input side",
                     "same_bits_as_dense": bool(torch.equal(ref, outs["dense"])),
                     "max_abs_difference": float((ref.double() - outs["dense"].double()).abs().max())}
            del outs, ref
            iters = {k: (200 if k != "dense" else (5 if n != 128 else 50)) for k in variants}
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, f in variants.items():  # alternating
                    f()
                    times[k].append(timed(torch, f, iters[k]))
            for k, v in times.items():
                point[k + "_ms"] = [round(t, 4) for t in v]
                point[k + "_ms_median"] = round(median(v), 4)
            nbytes = 2 * rows * cols * 2  # one read and one write of the fp16 matrix
            rate = nbytes / (point["op_ms_median"] * 1e-3)
            point["op_bytes"] = nbytes
            point["op_tb_per_s"] = round(rate / 1e12, 3)
            point["op_fraction_of_hbm_spec_8.0"] = round(rate / HBM_SPEC, 3)
            point["op_fraction_of_hbm_measured_6.29"] = round(rate / HBM_MEASURED, 3)
            point["fits_infinity_cache"] = bool(nbytes <= L3_BYTES)
            mine = "op_path" if transposed else "op"
            spread = max(max(times[k]) - min(times[k]) for k in (mine, "dense"))
            point["spread_ms"] = round(spread, 4)
            point["dense_over_op"] = round(point["dense_ms_median"] / point[mine + "_ms_median"], 1)
            point["op_wins_by_more_than_the_spread"] = bool(min(times["dense"]) - max(times[mine]) > spread)
            print(json.dumps(point))
            points.append(point)
            del variants
        del W
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "dtype": "float16", "points": points}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
