#!/usr/bin/env python3
"""Generate tests/golden/gptq_small.npz by running the REFERENCE's own GPTQ (QQQ/gptq/gptq.py, QQQ/gptq/quant.py) on the CPU.

Runs only where a checkout of the reference is present: pass its root.  The two modules are imported under a stub
package whose __path__ is the reference's QQQ/gptq directory, so its __init__ (which pulls in the CUDA packer) never runs; the only
patch is torch.cuda.synchronize, which fasterquant calls and a CPU-only torch refuses, and a wrapper around torch.linalg.cholesky that
keeps the upper factor fasterquant computes and does not return.  The outputs are committed as DATA (inputs and recorded results); no
reference source is copied.

One seeded 64 x 256 fp16 weight (two blocks, two groups) and 512 correlated calibration rows, in four settings: per-channel and g128,
mse off and on.  Stored: W, H and Hinv (upper triangles, packed), and per setting the codes (int8), the scales and s_extra.

usage: python tests/golden/gen_gptq_golden.py <reference root>
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
N, K, ROWS = 64, 256, 512


def load_reference(root):
    pkg = types.ModuleType("ref_gptq")
    pkg.__path__ = [os.path.join(root, "QQQ", "gptq")]
    sys.modules["ref_gptq"] = pkg
    return importlib.import_module("ref_gptq.gptq"), importlib.import_module("ref_gptq.quant")


def inputs():
    rng = np.random.Generator(np.random.PCG64(20241020))
    W = (rng.standard_normal((N, K)) * 0.02).astype(np.float16)
    mix = rng.standard_normal((K, K)) * (rng.random((K, K)) < 0.05) + np.eye(K)  # correlated columns
    X = (rng.standard_normal((ROWS, K)) * (0.2 + rng.random(K) * 2) @ mix).astype(np.float32)
    return W, X


def main():
    import gptq_ref

    if len(sys.argv) != 2:
        sys.exit(__doc__)
    root = sys.argv[1]
    gptq, quant = load_reference(root)
    torch.cuda.synchronize = lambda *a, **k: None
    kept = {}
    cholesky = torch.linalg.cholesky

    def keeping(A, *a, upper=False, **k):
        out = cholesky(A, *a, upper=upper, **k)
        if upper:
            kept["Hinv"] = out.clone()
        return out

    torch.linalg.cholesky = keeping
    W, X = inputs()
    iu = np.triu_indices(K)
    out = {"W": W}
    for gs in (-1, 128):
        for mse in (False, True):
            lin = torch.nn.Linear(K, N, bias=False).half()
            lin.weight.data = torch.from_numpy(W.copy())
            g = gptq.GPTQ(lin)
            g.quantizer = quant.Quantizer()
            g.quantizer.configure(4, perchannel=True, sym=True, mse=mse, groupsize=gs)
            for j in range(0, ROWS, 128):  # four samples of 128 rows, as four calibration sequences
                g.add_batch(torch.from_numpy(X[j:j + 128]), None)
            H = g.H.clone().numpy()
            scale, zero, g_idx, s_extra = g.fasterquant(percdamp=0.01, groupsize=gs)
            tag = f"g{gs}_mse{int(mse)}"
            wq = lin.weight.data.numpy()
            out[f"{tag}/codes"] = gptq_ref.codes(wq, scale.numpy(), gs != -1)
            out[f"{tag}/weight"] = wq
            out[f"{tag}/scales"] = scale.numpy().astype(np.float32)
            if s_extra is not None:
                out[f"{tag}/s_extra"] = s_extra.numpy().astype(np.float32)
            if "H_triu" not in out:
                out["H_triu"], out["Hinv_triu"] = H[iu], kept["Hinv"].numpy()[iu]
            else:
                assert np.array_equal(out["H_triu"], H[iu]) and np.array_equal(out["Hinv_triu"], kept["Hinv"].numpy()[iu])
    path = os.path.join(HERE, "gptq_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", len(out), "arrays")


if __name__ == "__main__":
    main()
