#!/usr/bin/env python3
"""Generate tests/golden/gptq_order_small.npz by running the REFERENCE's own GPTQ.fasterquant(actorder, static_groups) (QQQ/gptq/gptq.py,
QQQ/gptq/quant.py) on the CPU, the way gen_gptq_golden.py does: the two modules under a stub package, torch.cuda.synchronize patched
out, torch.linalg.cholesky wrapped to keep the upper factor, and here torch.argsort wrapped to record the first order it returns -- the
`perm` of act-order (the second call is its inverse).  The outputs are committed as DATA (inputs and recorded results); no reference
source is copied.

The inputs are gen_gptq_golden.py's seeded 64 x 256 fp16 weight and 512 calibration rows, with column 77 of the calibration zeroed -- a
dead column -- and W[::2, 77] = 0.2, so that in half the rows the dead column holds the row's maximum and its group's maximum: the
per-channel scales see it (they are found before the dead columns are zeroed), the static group scales do not (found after, and before
the permutation).  Five settings: per-channel act-order with mse off and on, g128 act-order + static groups with mse off and on, g128
static groups without act-order with mse off.  Stored: W, the triangle of H, perm, the triangle of the factor of the permuted Hessian
(and of the unpermuted one, for the setting without act-order), and per setting the codes (int8), weight, scales and s_extra.

usage: python tests/golden/gen_gptq_order_golden.py <reference root>
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
DEAD = 77
# (group size, act-order, static groups, mse)
SETTINGS = [(-1, True, False, False), (-1, True, False, True), (128, True, True, False), (128, True, True, True), (128, False, True, False)]


def tag_of(gs, act, static, mse):
    return f"g{gs}_act{int(act)}_static{int(static)}_mse{int(mse)}"


def inputs():
    import gen_gptq_golden as base

    W, X = base.inputs()
    X[:, DEAD] = 0
    W[::2, DEAD] = 0.2
    return W, X


def main():
    import gen_gptq_golden as base
    import gptq_ref

    if len(sys.argv) != 2:
        sys.exit(__doc__)
    gptq, quant = base.load_reference(sys.argv[1])
    torch.cuda.synchronize = lambda *a, **k: None
    kept = {}
    cholesky, argsort = torch.linalg.cholesky, torch.argsort

    def keeping(A, *a, upper=False, **k):
        out = cholesky(A, *a, upper=upper, **k)
        if upper:
            kept["Hinv"] = out.clone()
        return out

    def recording(*a, **k):
        out = argsort(*a, **k)
        kept.setdefault("perm", out.clone())
        return out

    torch.linalg.cholesky, torch.argsort = keeping, recording
    W, X = inputs()
    N, K = W.shape
    iu = np.triu_indices(K)
    out = {"W": W}
    for gs, act, static, mse in SETTINGS:
        kept.clear()
        lin = torch.nn.Linear(K, N, bias=False).half()
        lin.weight.data = torch.from_numpy(W.copy())
        g = gptq.GPTQ(lin)
        g.quantizer = quant.Quantizer()
        g.quantizer.configure(4, perchannel=True, sym=True, mse=mse, groupsize=gs)
        for j in range(0, X.shape[0], 128):  # four samples of 128 rows, as four calibration sequences
            g.add_batch(torch.from_numpy(X[j:j + 128]), None)
        H = g.H.clone().numpy()
        scale, zero, g_idx, s_extra = g.fasterquant(percdamp=0.01, groupsize=gs, actorder=act, static_groups=static)
        assert np.array_equal(g_idx.numpy(), np.arange(K) // (gs if gs != -1 else K))  # static groups: an ordinary checkpoint
        tag = tag_of(gs, act, static, mse)
        wq = lin.weight.data.numpy()
        out[f"{tag}/codes"] = gptq_ref.codes(wq, scale.numpy(), gs != -1)
        out[f"{tag}/weight"] = wq
        out[f"{tag}/scales"] = scale.numpy().astype(np.float32)
        if s_extra is not None:
            out[f"{tag}/s_extra"] = s_extra.numpy().astype(np.float32)
        if "H_triu" not in out:
            out["H_triu"] = H[iu]
        assert np.array_equal(out["H_triu"], H[iu])
        name = "Hinv_perm_triu" if act else "Hinv_triu"
        if act:
            if "perm" not in out:
                out["perm"] = kept["perm"].numpy().astype(np.int64)
            assert np.array_equal(out["perm"], kept["perm"].numpy())
        else:
            assert "perm" not in kept
        if name not in out:
            out[name] = kept["Hinv"].numpy()[iu]
        assert np.array_equal(out[name], kept["Hinv"].numpy()[iu])
    path = os.path.join(HERE, "gptq_order_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", len(out), "arrays")


if __name__ == "__main__":
    main()
