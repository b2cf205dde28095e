#!/usr/bin/env python3
"""Generate tests/golden/smooth_small.npz by running the REFERENCE's own migration classes (QQQ/smooth/migration/migration_llama.py:
Migrator1DRangeSearch, ...AWQ, ...SQ) on the CPU.

Runs only where a checkout of the reference is present: pass its root.  The module is imported under a stub package `QQQ` whose
`QQQ.smooth.migration.__path__` and `QQQ.smooth.quantization.__path__` are the reference's directories, so no __init__ of the reference
runs (a direct import fails on `easydict`); `QQQ.smooth.models.llama` is a stub that exposes transformers' apply_rotary_pos_emb and
repeat_kv, the two names the module functions use.  The outputs are committed as DATA (inputs and recorded results); no reference
source is copied.

Seeded inputs: 2 x 16 tokens, hidden 256, 4 heads (with 4 and with 2 KV heads), head_dim 64, intermediate 384, a few outlier channels
of both signs, one zero token row.  The weights lie on a grid of 2^-7 so that the committed file stays small.  Stored per kind (qkv, qkv_gqa, o_proj, up_and_gate,
down_proj), shared by both weight modes: x (fp16) and w_code (int8: w = w_code / 128 in fp16), the inputs; cos, sin for the qkv kinds
(the mask is causal_mask(16)); at, qx: three candidate indices (first, middle, last) and the reference's fake-quantised activation
there (the same in both modes: asserted); qw_rows.
Stored per case `<kind>_<pc|g128>` (method os+):
    scale           the reference's best scale (fp16)
    ranges, losses  every clipping range its walk visited (f64) and the loss there (f32)
    best, count     the index its walk ended on, and how many candidates it tried
    qw              the reference's fake-quantised weight at the three candidates `at`: its rows qw_rows, the first and last 16
    loss_bound      the largest RELATIVE per-candidate loss difference between mkldnn on and off on the generating machine: what the CPU's
                    choice of fp16 GEMM path can move a loss by.  The generator asserts that the best loss undercuts every other
                    candidate's by more than ten times that (relative), reseeding the case until it holds.
awq_o_proj_<mode> and sq_down_proj (on the inputs of those kinds): scale (and the ratios' losses, best) of the two other methods, for one kind each (awq in both weight modes:
without a clipping range the reference quantises the activation per group of 128, or per BATCH ELEMENT when the weight is per-channel).

The reference's export_smoothed_model and its calibration model classes (QQQ/smooth/models) are NOT driven: they reach into attributes
of transformers' attention modules (num_heads, num_key_value_heads, rotary_emb, causal_mask) that the installed transformers no longer
has.  tests/test_smooth_ref_cpu.py checks apply_smooth against literal per-tensor expectations instead.

usage: python tests/golden/gen_smooth_golden.py <reference root>
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
B, N, HIDDEN, HEADS, HEAD_DIM, INTER = 2, 16, 256, 4, 64, 384
W_GRID = 128  # weights are int8 codes / 128, stored as the codes


def load_reference(root):
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb, repeat_kv

    mods = {}
    for name, path in (("QQQ", None), ("QQQ.smooth", None), ("QQQ.smooth.models", None),
                       ("QQQ.smooth.migration", os.path.join(root, "QQQ", "smooth", "migration")),
                       ("QQQ.smooth.quantization", os.path.join(root, "QQQ", "smooth", "quantization"))):
        m = types.ModuleType(name)
        m.__path__ = [path] if path else []
        mods[name] = m
    llama = types.ModuleType("QQQ.smooth.models.llama")
    llama.apply_rotary_pos_emb, llama.repeat_kv = apply_rotary_pos_emb, repeat_kv
    mods["QQQ.smooth.models.llama"] = llama
    mods["QQQ.smooth.models"].llama = llama
    mods["QQQ.smooth"].models = mods["QQQ.smooth.models"]
    mods["QQQ"].smooth = mods["QQQ.smooth"]
    sys.modules.update(mods)
    return importlib.import_module("QQQ.smooth.migration.migration_llama")


def qconfigs(group):
    a = types.SimpleNamespace(quantizer="TokenFixedFakeQuantize", observer="MinMaxObserver", bit=8, symmetric=True, ch_axis=0)
    w = types.SimpleNamespace(quantizer="GroupFixedQuantize" if group else "FixedQuantize", observer="MinMaxObserver", bit=4, symmetric=True,
                              ch_axis=0, group_size=group or -1)
    return a, w


def inputs(kind, seed):
    g = torch.Generator().manual_seed(seed)
    K = INTER if kind == "down_proj" else HIDDEN
    rows = {"qkv": 3 * HIDDEN, "qkv_gqa": 2 * HIDDEN, "o_proj": HIDDEN, "up_and_gate": 2 * INTER, "down_proj": HIDDEN}[kind]
    x = torch.randn(B, N, K, generator=g)
    for j, f in ((5, 40.0), (K // 2 + 3, -25.0), (K - 7, 12.0), (77, -8.0)):
        x[:, :, j] = x[:, :, j].abs() * f
    x[1, 3] = 0
    w = torch.round(torch.randn(rows, K, generator=g) * 0.04 * W_GRID).clamp(-127, 127) / W_GRID  # on a grid: the committed file stays small
    return x.half(), w.half()


def extra_of(kind):
    import smooth_ref as R

    obs = torch.ones(B, N, dtype=torch.int64)
    if kind in ("qkv", "qkv_gqa"):
        kv = HEADS if kind == "qkv" else HEADS // 2
        e = R.make_extra(HEADS, kv, HEAD_DIM, N)
        return {"num_heads": HEADS, "num_key_value_heads": kv, "num_key_value_groups": HEADS // kv, "cos_cached": e["cos"][None],
                "sin_cached": e["sin"][None], "head_dim": HEAD_DIM, "attention_mask": e["mask"], "observation_mask": obs}, e
    if kind == "up_and_gate":
        return {"observation_mask": obs, "act_fn": torch.nn.functional.silu}, None
    return {"observation_mask": obs}, None


QW_ROWS = np.r_[0:16, -16:0]  # the weight rows whose fake-quantised values are stored (a row's bits depend on that row alone)


def run_os(M, kind, group, seed):
    """the reference's walk with every (range, loss) logged -> dict of arrays, or None where the best loss is not clear of the GEMM noise"""
    x, w = inputs(kind, seed)
    ref_extra, e = extra_of(kind)
    a_q, w_q = qconfigs(group)
    module_type = "qkv" if kind == "qkv_gqa" else kind
    logs = {}
    for flag in (True, False):
        with torch.backends.mkldnn.flags(enabled=flag):
            mig = M.Migrator1DRangeSearch(x.clone(), w.clone(), a_q, w_q, module_type, ref_extra)
            log = []
            inner = mig.cac_scale_loss
            mig.cac_scale_loss = lambda mn, mx, inner=inner, log=log: (log.append((mx, v := inner(mn, mx))), v)[1]
            scale = mig()
            logs[flag] = (scale, log, mig)
    scale, log, mig = logs[True]
    ranges = np.array([st for st, _ in log], dtype=np.float64)
    losses = np.array([v.item() for _, v in log], dtype=np.float32)
    off = np.array([v.item() for _, v in logs[False][1]], dtype=np.float32)
    bound = float(np.max(np.abs(losses.astype(np.float64) - off) / losses))
    best = 0
    for i in range(len(losses)):
        if losses[best] > losses[i]:
            best = i
    others = np.delete(losses.astype(np.float64), best)
    if not np.all((others - losses[best]) / losses[best] > 10 * bound) or np.any(others == losses[best]):
        return None
    assert torch.equal(scale, mig.cac_scale(torch.tensor(-ranges[best], dtype=torch.float16), torch.tensor(ranges[best], dtype=torch.float16)))
    at = np.array([0, len(ranges) // 2, len(ranges) - 1])
    qx, qw = [], []
    for i in at:
        mn, mx = torch.tensor(-ranges[i], dtype=torch.float16), torch.tensor(ranges[i], dtype=torch.float16)
        s = mig.cac_scale(mn, mx)
        qx.append(mig.quantize(x / s, mig.aob, (mn, mx)).numpy())
        qw.append(mig.quantize(w * s, mig.wob).numpy()[QW_ROWS])
    out = dict(scale=scale.numpy(), ranges=ranges, losses=losses, best=np.int64(best), count=np.int64(len(ranges)),
               at=at, qx=np.stack(qx), qw=np.stack(qw), loss_bound=np.float64(bound))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    M = load_reference(sys.argv[1])
    torch.set_num_threads(1)
    data, seeds = {}, {}
    for k, kind in enumerate(("qkv", "qkv_gqa", "o_proj", "up_and_gate", "down_proj")):
        for attempt in range(50):  # one seed per kind: both weight modes share the inputs
            seed = 1000 * k + attempt
            res = {group: run_os(M, kind, group, seed) for group in (0, 128)}
            if all(r is not None for r in res.values()):
                break
        else:
            raise SystemExit(f"{kind}: no seed gives a best loss clear of the GEMM noise")
        x, w = inputs(kind, seed)
        seeds[kind] = seed
        data.update({f"{kind}/x": x.numpy(), f"{kind}/w_code": (w.float() * W_GRID).numpy().astype(np.int8), f"{kind}/qx": res[0].pop("qx"),
                     f"{kind}/at": res[0].pop("at"), f"{kind}/seed": np.int64(seed), f"{kind}/qw_rows": QW_ROWS % w.shape[0]})
        e = extra_of(kind)[1]
        if e is not None:
            data.update({f"{kind}/cos": e["cos"].numpy(), f"{kind}/sin": e["sin"].numpy()})
        assert np.array_equal(res[128].pop("qx"), data[f"{kind}/qx"]) and np.array_equal(res[128].pop("at"), data[f"{kind}/at"])
        for group, r in res.items():
            tag = f"{kind}_{'g128' if group else 'pc'}"
            print(tag, "seed", seed, "count", int(r["count"]), "best", int(r["best"]), "bound", float(r["loss_bound"]))
            data.update({f"{tag}/{n}": v for n, v in r.items()})
    for group in (0, 128):  # awq, one kind, both weight modes
        x, w = inputs("o_proj", seeds["o_proj"])
        ref_extra, _ = extra_of("o_proj")
        a_q, w_q = qconfigs(group)
        mig = M.Migrator1DRangeSearchAWQ(x.clone(), w.clone(), a_q, w_q, "o_proj", ref_extra)
        log = []
        inner = mig.cac_scale_loss
        mig.cac_scale_loss = lambda s, inner=inner, log=log: (log.append(v := inner(s)), v)[1]
        scale = mig()
        tag = f"awq_o_proj_{'g128' if group else 'pc'}"
        losses = np.array([v.item() for v in log], dtype=np.float32)
        data.update({f"{tag}/scale": scale.numpy(), f"{tag}/losses": losses,
                     f"{tag}/best": np.int64(int(np.argmin(losses)))})
        print(tag, "best", int(np.argmin(losses)))
    x, w = inputs("down_proj", seeds["down_proj"])
    a_q, w_q = qconfigs(0)
    scale = M.Migrator1DRangeSearchSQ(x.clone(), w.clone(), a_q, w_q, "down_proj", extra_of("down_proj")[0])()
    data.update({"sq_down_proj/scale": scale.numpy()})
    out = os.path.join(HERE, "smooth_small.npz")
    np.savez_compressed(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
