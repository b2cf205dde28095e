"""The N>1 path of bench.py (M-sharded GEMM + chunk-pipelined all-gather, qqq_amd/parallel.py) end to end on
real kernels: two ranks share cuda:0 and talk over gloo (RCCL refuses two ranks on one device; the 8-GPU RCCL
run is the driver's).  `--check` makes every rank compare the gathered outputs with a local full GEMM."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_ranks_one_gpu_gloo(dev):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, QQQ_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--full", "--no-cpu", "--no-fp16", "--check"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "identical to local full GEMMs" in p.stderr
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["value"] > 0
    # GEMM-only, all-gather-only and overlapped totals of the sharded points; the M=4096 point is pipelined
    mg = out["multi_gpu"]["4096"]
    assert mg["chunks"] >= 2 and mg["rows_per_rank"] == 2048
    assert all(mg[k] > 0 for k in ("gemm_only_us", "allgather_only_us", "overlapped_us"))
    # what lets a reader verify an N > 1 line: the collective really spanned N ranks, over which backend, and how the step was launched
    assert out["multi_gpu"]["world_seen"] == 2 and out["multi_gpu"]["backend"] == "gloo" and out["multi_gpu"]["launch"] == "eager"
    assert out["config"]["launch"] == "eager" and "M-sharded over 2 GPUs" in out["config"]["parallelism"]
    assert len(line) < 4000  # the N > 1 line is bounded like the N = 1 one (the driver keeps an 8 KB tail)


def test_bench_two_ranks_rccl_when_two_gpus():
    """The same path over RCCL (torch "nccl" backend) when the box has >= 2 GPUs: so that the driver's 8-GPU run is not
    the first RCCL execution of the in-place all_gather_into_tensor pipeline.  Skips on 1-GPU boxes."""
    import torch

    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("QQQ_BENCH_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--no-cpu", "--no-fp16", "--check"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "identical to local full GEMMs" in p.stderr


@pytest.mark.parametrize("extra", [{}, {"QQQ_BENCH_NGRAPH": "1"}, {"QQQ_BENCH_SMS": "224"}], ids=["eager", "hipgraph", "sms224"])
def test_bench_one_rank_rccl_through_the_sharded_path(dev, extra):
    """ONE rank over RCCL (torch "nccl") through bench.py's N > 1 code path (QQQ_BENCH_FORCE_DIST=1): process group on a 1-GPU box, the
    M-sharded GEMM, the in-place all_gather_into_tensor on the side stream, --check -- eagerly, captured into a hipGraph (QQQ_BENCH_NGRAPH=1)
    and with the GEMMs capped to 224 CUs on the library's CU-masked stream beside RCCL's stream (QQQ_BENCH_SMS) -- so that the driver's
    8-GPU run is not the first time RCCL, the capture and the masked stream meet this code.  No curve: a smoke."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, QQQ_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", **extra)
    env.pop("QQQ_BENCH_BACKEND", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu", "--no-fp16",
           "--check"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "identical to local full GEMMs" in p.stderr
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 1 and out["value"] > 0
    mg = out["multi_gpu"]
    assert mg["world_seen"] == 1 and mg["backend"].startswith("nccl")
    assert all(mg["4096"][k] > 0 for k in ("gemm_only_us", "allgather_only_us", "overlapped_us"))
    if "QQQ_BENCH_NGRAPH" in extra:
        assert "hipGraph" in mg["launch"], mg["launch"]   # the capture of the collective really held
    else:
        assert mg["launch"] == "eager"
    assert len(line) < 4000
