#!/usr/bin/env python3
"""Generate tests/golden/rotate_k_small.npz by running the REFERENCE's own rotation (QQQ/rotation/rotation.py, hadamard_utils.py) on the
CPU at hidden sizes K * 2^p, where its Q is diag(s) (hadK^T (x) H_m) / d with hadK one of its literal tables.

Runs only where a checkout of the reference is present: pass its root.  The reference is imported by the stubs of gen_rotate_golden.py
(no __init__ of it runs, Tensor.cuda is the identity) and fed the same stand-in module objects.  The outputs are committed as DATA
(inputs and recorded results); no reference source and no table of it is copied: the tests recover each K x K table from the recorded Q.

(a) One seeded 2-layer Qwen2-style model (hidden 96 = 12 * 8, 6 heads, 2 KV heads, head_dim 16, intermediate 64, vocab 48, q/k/v biases,
    untied, fp16).  Stored: orig/<name> every tensor; signs (the seeded randint of the reference's random_hadamard_matrix replayed -- NOT
    read from Q[:, 0]: row 0 of the tables is not all ones) and the reference's Q; fused/<name> what fuse_layer_norms changed;
    rotq/<name> what the Q stage changed (rotate_embeddings ... rotate_mlp_output).  The per-head stage is not run: it is the power-of-two
    op, which tests/golden/rotate_small.npz covers.
(b) had<n>/{W, signs, Q, out}: one 32 x n fp16 matrix through the reference's rotate_embeddings with its Q, at n = 112 (28 * 4),
    160 (40 * 4), 24 (12 * 2), 12 (12 * 1: no Sylvester stage) and 20 (20 * 1: K = 20 occurs only at m = 1).

Asserted here: every Q has the Kronecker structure (the table recovered from it, tests/rotate_k_ref.py's hadamard_matrix_k, gives Q
back bit for bit, and the table is Hadamard).  The reference's f64 matmul rounds every product w * q and then the sums; the op divides
the exact sum once.  COUNTED here, not assumed: mismatches/<case> is the number of fp16 elements where tests/rotate_k_ref.py and the
reference differ, max_ulp/<case> the largest such difference in fp16 ulps.

usage: python tests/golden/gen_rotate_k_golden.py <reference root>
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import gen_rotate_golden as G  # noqa: E402

HIDDEN, HEADS, KV_HEADS, HEAD_DIM, INTER, VOCAB, LAYERS, K = 96, 6, 2, 16, 64, 48, 2, 12
SEED = 20241021
CASES = ((112, 28), (160, 40), (24, 12), (12, 12), (20, 20))


def reference_q(rotation, n, seed):
    """the reference's Q and the signs it drew: the first draw of random_hadamard_matrix after the seed, replayed"""
    torch.manual_seed(seed)
    Q = rotation.get_orthogonal_matrix(n, "hadamard", torch.device("cpu"))
    torch.manual_seed(seed)
    signs = (torch.randint(low=0, high=2, size=(n,)) * 2 - 1).numpy().astype(np.int8)
    return Q.numpy(), signs


def structure(Q, signs, k):
    """assert Q = diag(s) (table^T (x) H_m) / d for the table recovered from it, and that the table is Hadamard"""
    import rotate_k_ref as RK

    table = RK.recover_table(Q, signs, k)
    t = table.astype(np.int64)
    assert np.array_equal(t @ t.T, k * np.eye(k, dtype=np.int64)), "the recovered table is not Hadamard"
    mine = RK.hadamard_matrix_k(signs, table, Q.shape[0] // k)
    assert np.array_equal(mine.view(np.uint64), np.ascontiguousarray(Q).view(np.uint64)), "Q has not the Kronecker structure"
    return table


def distance(mine, theirs):
    diff = mine.view(np.uint16) != theirs.view(np.uint16)
    if not diff.any():
        return 0, 0
    ulp = np.spacing(np.maximum(np.abs(mine), np.abs(theirs)).astype(np.float16)).astype(np.float64)
    return int(diff.sum()), int(np.ceil((np.abs(mine.astype(np.float64) - theirs.astype(np.float64)) / ulp)[diff].max()))


def main():
    import rotate_k_ref as RK

    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rotation, _ = G.load_reference(sys.argv[1])
    G.HIDDEN, G.HEADS, G.KV_HEADS, G.HEAD_DIM, G.INTER, G.VOCAB, G.LAYERS = HIDDEN, HEADS, KV_HEADS, HEAD_DIM, INTER, VOCAB, LAYERS
    sd = G.make_state_dict()
    model = G.make_model(sd)
    orig = G.snapshot(model)
    out = {"orig/" + k: v for k, v in orig.items()}

    rotation.fuse_layer_norms(model)
    fused = G.snapshot(model)
    out.update({"fused/" + k: v for k, v in G.changed(orig, fused).items()})

    Q, signs = reference_q(rotation, HIDDEN, SEED)
    table = structure(Q, signs, K)
    out["signs"], out["Q"] = signs, Q
    Qt = torch.from_numpy(Q)
    with torch.inference_mode():
        rotation.rotate_embeddings(model, Qt, "qwen2", "cpu")
        rotation.rotate_head(model, Qt, "qwen2", "cpu")
        for layer in model.model.layers:
            rotation.rotate_attention_inputs(layer, Qt, "qwen2", "cpu")
            rotation.rotate_attention_output(layer, Qt, "qwen2", "cpu")
            rotation.rotate_mlp_input(layer, Qt, "qwen2", "cpu")
            rotation.rotate_mlp_output(layer, Qt, "qwen2", "cpu")
        rotq = G.snapshot(model)
    out.update({"rotq/" + k: v for k, v in G.changed(fused, rotq).items()})
    mine = RK.rotate_q(fused, HIDDEN, signs, table)
    bad, worst = 0, 0
    for k in rotq:
        b, w = distance(mine[k], rotq[k])
        bad, worst = bad + b, max(worst, w)
    out["mismatches/model"], out["max_ulp/model"] = np.int64(bad), np.int64(worst)
    report = [("model", bad, worst)]

    for n, k in CASES:
        Qn, sn = reference_q(rotation, n, n)
        tn = structure(Qn, sn, k)
        W = np.random.Generator(np.random.PCG64(n)).standard_normal((32, n)).astype(np.float16)
        emb = torch.nn.Module()
        emb.model = torch.nn.Module()
        emb.model.embed_tokens = torch.nn.Embedding(32, n).half()
        emb.model.embed_tokens.weight.data = torch.from_numpy(W.copy())
        with torch.inference_mode():
            rotation.rotate_embeddings(emb, torch.from_numpy(Qn), "qwen2", "cpu")
        theirs = emb.model.embed_tokens.weight.data.numpy().copy()
        tag = f"had{n}"
        out[tag + "/W"], out[tag + "/Q"], out[tag + "/signs"], out[tag + "/out"] = W, Qn, sn, theirs
        b, w = distance(RK.hadamard_rows_k(W, n // k, tn, sn), theirs)
        out["mismatches/" + tag], out["max_ulp/" + tag] = np.int64(b), np.int64(w)
        report.append((tag, b, w))

    path = os.path.join(HERE, "rotate_k_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", len(out), "arrays; (case, mismatches, worst ulp):", report)


if __name__ == "__main__":
    main()
