"""bench.py's pure host logic (no GPU): the timed region replays EXACTLY K steps whatever the graph batching, and the algorithmic
work / byte counts are SURVEY 8d's."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_graph_schedule_replays_exactly_k_steps():
    import bench

    for steps in range(0, 130):
        for spg in (1, 2, 3, 5, 10, 16):
            sc = bench.graph_schedule(steps, spg)
            assert sum(sc) == steps, (steps, spg, sc)
            assert all(1 <= n <= max(spg, 1) for n in sc), (steps, spg, sc)
            if steps and spg > 1:
                assert sc[0] == 1 and len(set(sc)) <= 3, (steps, spg, sc)  # one-step opener; at most three graphs to capture
    assert bench.graph_schedule(20, 10) == [1, 9, 10]  # the driver's K
    assert bench.graph_schedule(100, 10) == [1, 9] + [10] * 9


def test_algorithmic_work_is_the_surveys():
    import bench

    N, K = bench.N_FULL, bench.K_FULL
    assert (N, K) == (8192, 21760) and tuple(bench.SWEEP_M) == (1, 16, 128, 1024, 4096)
    for M, ops, b_pc, b_g in ((1, 0.357e9, 89_199_876, 91_985_156), (4096, 1460.29e9, 245_415_936, 248_201_216)):
        assert abs(bench.algorithmic_ops(M, N, K) - ops) / ops < 2e-3
        assert bench.algorithmic_bytes(M, N, K, False) == b_pc and bench.algorithmic_bytes(M, N, K, True) == b_g


def _worst_case_result():
    """round 4's full 21 KB result (the one the driver could not parse) + an N > 1 block + pessimistic float lengths"""
    import json

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = json.load(open(os.path.join(root, "profiles", "r04_bench_final.json")))
    d["multi_gpu"] = {str(M): {"gemm_only_us": 123.456789012345, "allgather_only_us": 98.7654321098765, "overlapped_us": 150.123456789012,
                               "chunks": 4, "rows_per_rank": M // 8} for M in (1024, 4096)}
    d["multi_gpu"].update(world_seen=8, backend="nccl (RCCL)", launch="eager (hipGraph capture failed on at least one rank)")
    d["detail"] = "gpurun_out/bench_detail_n8.json"
    d["device"] = "AMD Instinct MI355X " * 2
    return d


def test_printed_line_is_bounded_and_carries_the_contract():
    """the driver keeps an 8 KB stdout tail: the printed line must stay far below it and still hold every contract key,
    `roofline` and `cpu_baseline` (BENCH_r04.parsed = null)"""
    import json

    import bench

    full = _worst_case_result()
    assert len(json.dumps(full)) > 15000  # the input really is the oversized one
    line = bench.compact_line(full)
    assert "\n" not in line and len(line) < bench.LINE_LIMIT <= 4000, len(line)
    out = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "roofline_hbm", "cpu_baseline", "per_m", "per_m_g128", "llama7b"):
        assert k in out, k
    assert "workload" in out["config"] and "model" not in out["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in out["roofline"] and k in out["roofline_hbm"], k
    assert abs(out["roofline"]["frac"] - full["roofline"]["frac"]) < 1e-4
    assert abs(out["roofline"]["achieved"] / out["roofline"]["peak"] - out["roofline"]["frac"]) < 1e-3
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in out["cpu_baseline"], k
    assert set(out["per_m"]) == {"1", "16", "128", "1024", "4096"}
    assert abs(out["value"] - full["value"]) / full["value"] < 1e-4


def test_printed_line_survives_pathological_blocks():
    """an optional block that explodes (say, a per-layer table leaking into llama7b) is dropped, never the contract keys"""
    import json

    import bench

    full = _worst_case_result()
    full["llama7b"]["sum_of_7_linears"]["per_channel"] = {str(i): {"quantlinear_us": 1.0 / 3, "speedup": 2.0 / 3} for i in range(400)}
    line = bench.compact_line(full)
    assert len(line) < bench.LINE_LIMIT
    out = json.loads(line)
    assert "roofline" in out and "cpu_baseline" in out and out["llama7b"] == {"dropped": "see detail file"}


def test_dump_outputs_is_seeded_and_bounded(tmp_path):
    """--dump-outputs: the row sample of a large output is fixed run to run, the whole sweep stays under 64 MB, and what is
    written is float32 holding exactly the fp16 values of the sampled rows"""
    import numpy as np
    import torch

    import bench

    r = bench.dump_rows(4096)
    assert np.array_equal(r, bench.dump_rows(4096)) and len(r) == bench.DUMP_MAX_ROWS
    assert np.all(np.diff(r) > 0) and r[0] >= 0 and r[-1] < 4096
    assert np.array_equal(bench.dump_rows(16), np.arange(16))
    total = sum(len(bench.dump_rows(M)) * bench.N_FULL * 4 + (8 * bench.DUMP_MAX_ROWS if M > bench.DUMP_MAX_ROWS else 0)
                for M in bench.SWEEP_M)
    assert total <= 64 * 2**20, total

    g = torch.Generator().manual_seed(1)
    big = torch.randn((bench.DUMP_MAX_ROWS + 88, 8), generator=g).half()
    small = torch.randn((3, 8), generator=g).half()
    n = bench.dump_outputs(str(tmp_path), {"D_big": big, "D_small": small})
    got_big, got_small = np.load(tmp_path / "D_big.npy"), np.load(tmp_path / "D_small.npy")
    rows = np.load(tmp_path / "D_big_rows.npy")
    assert got_big.dtype == np.float32 and got_small.dtype == np.float32 and rows.dtype == np.float64
    assert np.array_equal(rows, bench.dump_rows(big.shape[0]))
    assert np.array_equal(got_big, big.float().numpy()[rows.astype(np.int64)])
    assert np.array_equal(got_small, small.float().numpy())
    assert n == got_big.nbytes + got_small.nbytes + rows.nbytes
    assert sorted(p.name for p in tmp_path.iterdir()) == ["D_big.npy", "D_big_rows.npy", "D_small.npy"]


def test_full_is_opt_in():
    """a plain run measures the headline only; everything else waits for --full"""
    import bench

    assert bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"]).full is False
    assert bench.parse_args(["--full"]).full is True


def test_plain_line_carries_the_contract():
    """the line of a plain run (no --full blocks in the result) still holds every contract key and nothing it did not measure"""
    import json

    import bench

    full = _worst_case_result()
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "timed_region_ms", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "device")
    plain = {k: full[k] for k in keep}
    out = json.loads(bench.compact_line(plain))
    for k in keep:
        assert k in out, k
    for k in ("roofline", "roofline_hbm", "per_m", "per_m_g128", "llama7b", "cpu_baseline", "eager_ms_per_step", "step_us_median", "detail"):
        assert k not in out, k
    assert out["value"] == bench._r(full["value"]) and out["ms_per_step"] == bench._r(full["ms_per_step"])
