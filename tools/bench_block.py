#!/usr/bin/env python3
"""What the norm / activation / quantiser launches around the W4A8 GEMMs cost per Llama-2-7B decoder layer (hidden 4096, intermediate 11008),
unfused (torch expressions + QuantLinear.forward, which quantises its own fp16 input) against fused (rmsnorm_quant / silu_mul_quant feeding
QuantLinear.forward_int8).  Every path is replayed from a hipGraph (tools/bench_llama.time_fn), per-channel and g128, m in {1, 16, 128, 1024, 4096}:

    attn_in   input_layernorm (with the residual add) + the fused q|k|v projection
        unfused     h = residual + x; y = LlamaRMSNorm(h) in torch;                     qkv.forward(y)
        fused       QuantRMSNorm(x, residual) -> (xq, s1);                             qkv.forward_int8(xq, s1)
    mlp       post_attention_layernorm (with the residual add) + the MLP
        unfused     torch norm; gate.forward(y), up.forward(y); F.silu(g) * u;          down.forward(.)
        fused       QuantRMSNorm; QuantLlamaMLP.forward_int8 (gate / up forward_int8, silu_mul_quant, down forward_int8)
        unfused_gu  torch norm; gate_up.forward(y) (fuse_quant_linears); silu * up of the halves; down.forward(.)
        fused_gu    QuantRMSNorm; QuantLlamaMLP.forward_int8 after fuse_gate_up()

    python tools/bench_block.py [--m 1,16,...] [--out FILE]   -> one JSON object on stdout
    python tools/bench_block.py --summarize TRACE_DIR          -> per-kernel times and HBM fractions from a rocprofv3 --kernel-trace run of the above
"""
import argparse
import collections
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIDDEN, INTER, EPS = 4096, 11008, 1e-5
MS = (1, 16, 128, 1024, 4096)
HBM_BYTES_PER_S = 8e12


def torch_rmsnorm(h, w):
    # LlamaRMSNorm.forward (transformers) on fp16
    import torch

    hs = h.to(torch.float32)
    hs = hs * torch.rsqrt(hs.pow(2).mean(-1, keepdim=True) + EPS)
    return w * hs.to(torch.float16)


def run(ms, group_sizes):
    import torch
    import torch.nn.functional as F

    from bench_llama import make_ql, time_fn
    from qqq_amd import QuantLlamaMLP, QuantRMSNorm, fuse_quant_linears

    dev = torch.device("cuda:0")
    out = {"hidden": HIDDEN, "intermediate": INTER, "unit": "us per call, hipGraph replay (median)", "points": []}
    for gs in group_sizes:
        qkv = make_ql(dev, 3 * HIDDEN, HIDDEN, gs, seed=1)
        mlp = QuantLlamaMLP(HIDDEN, INTER, gs).to(dev)
        mlp.gate_proj, mlp.up_proj, mlp.down_proj = make_ql(dev, INTER, HIDDEN, gs, 2), make_ql(dev, INTER, HIDDEN, gs, 3), make_ql(dev, HIDDEN, INTER, gs, 4)
        gate_up = fuse_quant_linears([mlp.gate_proj, mlp.up_proj])
        mlp_gu = QuantLlamaMLP(HIDDEN, INTER, gs).to(dev)
        mlp_gu.gate_proj, mlp_gu.up_proj, mlp_gu.down_proj = mlp.gate_proj, mlp.up_proj, mlp.down_proj
        mlp_gu.fuse_gate_up()
        norm = QuantRMSNorm(HIDDEN, eps=EPS).to(dev)
        norm.weight.data = (1 + 0.1 * torch.randn(HIDDEN, device=dev)).half()
        w = norm.weight
        for m in ms:
            x = (torch.randn((m, HIDDEN), device=dev) * 0.01).half()  # the residual grows by x per replay: keep it small
            res = torch.randn((m, HIDDEN), device=dev).half()

            def attn_unfused():
                h = res + x
                return qkv.forward(torch_rmsnorm(h, w))

            def attn_fused():
                return qkv.forward_int8(*norm(x, res))

            def mlp_unfused():
                y = torch_rmsnorm(res + x, w)
                return mlp.down_proj.forward(F.silu(mlp.gate_proj.forward(y)) * mlp.up_proj.forward(y))

            def mlp_unfused_gu():
                gu = gate_up.forward(torch_rmsnorm(res + x, w))
                return mlp.down_proj.forward(F.silu(gu[:, :INTER]) * gu[:, INTER:])

            def mlp_fused():
                return mlp.forward_int8(*norm(x, res))

            def mlp_fused_gu():
                return mlp_gu.forward_int8(*norm(x, res))

            pt = {"group_size": gs, "m": m}
            for name, fn in (("attn_in_unfused", attn_unfused), ("attn_in_fused", attn_fused), ("mlp_unfused", mlp_unfused),
                             ("mlp_fused", mlp_fused), ("mlp_unfused_gu", mlp_unfused_gu), ("mlp_fused_gu", mlp_fused_gu)):
                pt[name] = round(time_fn(fn), 2)
            pt["attn_in_saved"] = round(pt["attn_in_unfused"] - pt["attn_in_fused"], 2)
            pt["mlp_saved"] = round(pt["mlp_unfused"] - pt["mlp_fused"], 2)
            pt["mlp_gu_saved"] = round(pt["mlp_unfused_gu"] - pt["mlp_fused_gu"], 2)
            out["points"].append(pt)
            print(json.dumps(pt), file=sys.stderr, flush=True)
    return out


def _k_of(name):
    # the row length behind a kernel instance in THIS tool's runs: the <VPT, NT> instances that cover k = 4096 (VPT * NT * 8 == 4096) are only
    # launched for the hidden size, every other instance for the intermediate size (include/qqq_amd_act.h dispatch: act_launch in qqq_w4a8.hip, shared with qqq_dynamic_quant)
    vpt, nt = (int(v) for v in name.split("<")[1].rstrip(">").split(","))
    return HIDDEN if vpt * nt * 8 == HIDDEN else INTER


def summarize(trace_dir):
    from code_object import _demangle

    times = collections.defaultdict(list)
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            name = name[5:] if name.startswith("void ") else name
            name = name.split("(")[0]
            name = _demangle(name) if name.startswith("_Z") else name
            fam = name.split("<")[0]
            if fam not in ("qqq_rmsnorm_quant_kernel", "qqq_silu_mul_quant_kernel", "qqq_dynamic_quant_kernel"):
                continue
            m = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
            times[(fam, _k_of(name), m)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    rows = []
    for (fam, k, m), v in sorted(times.items()):
        v = sorted(v)
        med = v[len(v) // 2]
        if fam == "qqq_rmsnorm_quant_kernel":  # x + residual read, residual + xq written (y not stored on the fused path), s1
            nbytes = m * k * (2 + 2 + 1 + 2) + 4 * m
        elif fam == "qqq_silu_mul_quant_kernel":  # gate + up read, xq written, s1
            nbytes = m * k * (2 + 2 + 1) + 4 * m
        else:  # x read, xq written, s1
            nbytes = m * k * (2 + 1) + 4 * m
        rows.append({"kernel": fam, "k": k, "m": m, "calls": len(v), "median_us": round(med, 2), "min_us": round(v[0], 2),
                     "bytes": nbytes, "hbm_fraction_of_8TBps": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 4)})
    return {"unit": "kernel time from rocprofv3 --kernel-trace (median over calls)", "kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", default=",".join(map(str, MS)))
    ap.add_argument("--group-sizes", default="-1,128")
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarize", default=None, metavar="TRACE_DIR")
    a = ap.parse_args()
    if a.summarize:
        res = summarize(a.summarize)
    else:
        res = run([int(v) for v in a.m.split(",")], [int(v) for v in a.group_sizes.split(",")])
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
