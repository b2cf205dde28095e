#!/usr/bin/env python3
"""Generate tests/golden/rotate_small.npz by running the REFERENCE's own rotation (QQQ/rotation/rotation.py, hadamard_utils.py) on the CPU.

Runs only where a checkout of the reference is present: pass its root.  The two modules are imported under a stub package `QQQ` whose
`QQQ.rotation.__path__` is the reference's directory, so no __init__ of the reference runs; `QQQ.utils` is a stub with the seven
accessors rotation.py imports (model.model.layers and the like), `tqdm` is a pass-through where it is missing, and Tensor.cuda is
patched to the identity.  The reference's functions are fed small stand-in module objects (torch.nn.Linear / Embedding and a norm with a
weight and no bias).  The outputs are committed as DATA (inputs and recorded results); no reference source is copied.

THE STAND-IN.  The per-head step of the reference calls fast_hadamard_transform.hadamard_transform, a CUDA package that is not here.
It is replaced by that package's documented meaning, `x @ H * scale` with H the Sylvester matrix, as an f32 matrix product: a STAND-IN
for the package's f32 butterfly, not its bits.  Everything it touched is stored under keys that begin with `full_standin/`; `Q`,
`fused/`, `rotq/` and `had128/` are the reference's own arithmetic alone.

One seeded 2-layer Qwen2-style model (hidden 64, 4 heads, 2 KV heads, head_dim 16, intermediate 128, vocab 96, q/k/v biases, untied,
fp16).  Stored: orig/<name> every tensor; signs and the reference's Q; fused/<name> what fuse_layer_norms changed; rotq/<name> what the
Q stage changed (rotate_embeddings ... rotate_mlp_output); full_standin/<name> what rotate_ov_proj changed after it;
standin_mismatches: how many elements of full_standin/ differ from tests/rotate_ref.py's per-head step (each by at most
standin_max_ulp fp16 ulps); had128/{W, signs, Q, out}: one 32 x 128 fp16 matrix through the reference's rotate_embeddings with its Q for
n = 128, the inexact divisor.

usage: python tests/golden/gen_rotate_golden.py <reference root>
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
HIDDEN, HEADS, KV_HEADS, HEAD_DIM, INTER, VOCAB, LAYERS = 64, 4, 2, 16, 128, 96, 2


def sylvester(n):
    i = np.arange(n)
    bits = i[:, None] & i[None, :]
    par = np.zeros_like(bits)
    while bits.any():
        par ^= bits & 1
        bits >>= 1
    return torch.from_numpy((1 - 2 * par).astype(np.float32))


def standin_hadamard_transform(x, scale=1.0):
    """STAND-IN for fast_hadamard_transform.hadamard_transform: its documented meaning, in f32"""
    return (x.float() @ sylvester(x.shape[-1])) * torch.as_tensor(scale, dtype=torch.float32)


def load_reference(root):
    qqq = types.ModuleType("QQQ")
    qqq.__path__ = []
    utils = types.ModuleType("QQQ.utils")
    utils.get_model_architecture = lambda config: "qwen2"
    utils.get_transformer_layers = lambda model, model_type: list(model.model.layers)
    utils.get_pre_head_layernorm = lambda model, model_type: model.model.norm
    utils.get_lm_head = lambda model, model_type: model.lm_head
    utils.get_embeddings = lambda model, model_type: [model.model.embed_tokens]
    utils.free_memory = lambda: None
    utils.str2torch_device = lambda device: torch.device("cpu")
    rot = types.ModuleType("QQQ.rotation")
    rot.__path__ = [os.path.join(root, "QQQ", "rotation")]
    fht = types.ModuleType("fast_hadamard_transform")
    fht.hadamard_transform = standin_hadamard_transform
    sys.modules.update({"QQQ": qqq, "QQQ.utils": utils, "QQQ.rotation": rot, "fast_hadamard_transform": fht})
    try:
        import tqdm  # noqa: F401
    except ImportError:
        t = types.ModuleType("tqdm")
        t.tqdm = lambda it, **k: it
        sys.modules["tqdm"] = t
    torch.Tensor.cuda = lambda self, *a, **k: self
    return importlib.import_module("QQQ.rotation.rotation"), importlib.import_module("QQQ.rotation.hadamard_utils")


class Norm(torch.nn.Module):
    def __init__(self, weight):
        super().__init__()
        self.weight = torch.nn.Parameter(weight, requires_grad=False)


def linear(weight, bias=None):
    m = torch.nn.Linear(weight.shape[1], weight.shape[0], bias=bias is not None).half()
    m.weight.data = weight.clone()
    if bias is not None:
        m.bias.data = bias.clone()
    return m


def make_state_dict():
    rng = np.random.Generator(np.random.PCG64(20241021))

    def w(rows, cols):
        return (rng.standard_normal((rows, cols)) / np.sqrt(cols)).astype(np.float16)

    def norm():
        return (1 + 0.25 * rng.standard_normal(HIDDEN)).astype(np.float16)

    sd = {"model.embed_tokens.weight": (rng.standard_normal((VOCAB, HIDDEN))).astype(np.float16)}
    for i in range(LAYERS):
        p = f"model.layers.{i}."
        for name, rows in (("q", HEADS * HEAD_DIM), ("k", KV_HEADS * HEAD_DIM), ("v", KV_HEADS * HEAD_DIM)):
            sd[p + f"self_attn.{name}_proj.weight"] = w(rows, HIDDEN)
            sd[p + f"self_attn.{name}_proj.bias"] = (0.1 * rng.standard_normal(rows)).astype(np.float16)
        sd[p + "self_attn.o_proj.weight"] = w(HIDDEN, HEADS * HEAD_DIM)
        sd[p + "mlp.gate_proj.weight"] = w(INTER, HIDDEN)
        sd[p + "mlp.up_proj.weight"] = w(INTER, HIDDEN)
        sd[p + "mlp.down_proj.weight"] = w(HIDDEN, INTER)
        sd[p + "input_layernorm.weight"] = norm()
        sd[p + "post_attention_layernorm.weight"] = norm()
    sd["model.norm.weight"] = norm()
    sd["lm_head.weight"] = w(VOCAB, HIDDEN)
    return sd


def make_model(sd):
    t = {k: torch.from_numpy(v.copy()) for k, v in sd.items()}
    model = torch.nn.Module()
    model.config = types.SimpleNamespace(hidden_size=HIDDEN, num_attention_heads=HEADS, architectures=["Qwen2ForCausalLM"])
    model.model = torch.nn.Module()
    model.model.embed_tokens = torch.nn.Embedding(VOCAB, HIDDEN).half()
    model.model.embed_tokens.weight.data = t["model.embed_tokens.weight"]
    layers = []
    for i in range(LAYERS):
        p = f"model.layers.{i}."
        layer = torch.nn.Module()
        layer.self_attn = torch.nn.Module()
        for name in "qkv":
            setattr(layer.self_attn, name + "_proj", linear(t[p + f"self_attn.{name}_proj.weight"], t[p + f"self_attn.{name}_proj.bias"]))
        layer.self_attn.o_proj = linear(t[p + "self_attn.o_proj.weight"])
        layer.mlp = torch.nn.Module()
        for name in ("gate", "up", "down"):
            setattr(layer.mlp, name + "_proj", linear(t[p + f"mlp.{name}_proj.weight"]))
        layer.input_layernorm = Norm(t[p + "input_layernorm.weight"])
        layer.post_attention_layernorm = Norm(t[p + "post_attention_layernorm.weight"])
        layers.append(layer)
    model.model.layers = torch.nn.ModuleList(layers)
    model.model.norm = Norm(t["model.norm.weight"])
    model.lm_head = linear(t["lm_head.weight"])
    return model


def snapshot(model):
    return {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}


def changed(before, after):
    return {k: v for k, v in after.items() if not np.array_equal(v.view(np.uint16), before[k].view(np.uint16))}


def main():
    import rotate_ref

    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rotation, had = load_reference(sys.argv[1])
    sd = make_state_dict()
    model = make_model(sd)
    orig = snapshot(model)
    assert set(orig) == set(sd) and all(np.array_equal(orig[k], sd[k]) for k in sd)
    out = {"orig/" + k: v for k, v in orig.items()}

    rotation.fuse_layer_norms(model)
    fused = snapshot(model)
    out.update({"fused/" + k: v for k, v in changed(orig, fused).items()})

    torch.manual_seed(20241021)
    Q = rotation.get_orthogonal_matrix(HIDDEN, "hadamard", torch.device("cpu"))
    signs = np.sign(Q[:, 0].numpy()).astype(np.int8)  # Q = diag(s) H / d and H[:, 0] = 1
    out["signs"], out["Q"] = signs, Q.numpy()
    with torch.inference_mode():
        rotation.rotate_embeddings(model, Q, "qwen2", "cpu")
        rotation.rotate_head(model, Q, "qwen2", "cpu")
        for layer in model.model.layers:
            rotation.rotate_attention_inputs(layer, Q, "qwen2", "cpu")
            rotation.rotate_attention_output(layer, Q, "qwen2", "cpu")
            rotation.rotate_mlp_input(layer, Q, "qwen2", "cpu")
            rotation.rotate_mlp_output(layer, Q, "qwen2", "cpu")
        rotq = snapshot(model)
        for layer in model.model.layers:
            rotation.rotate_ov_proj(layer, "qwen2", HEADS, HIDDEN // HEADS)
        full = snapshot(model)
    out.update({"rotq/" + k: v for k, v in changed(fused, rotq).items()})
    out.update({"full_standin/" + k: v for k, v in changed(rotq, full).items()})

    # how far the stand-in's f32 product is from the exact sum rounded once (tests/rotate_ref.py), counted, not assumed
    ours = rotate_ref.rotate_ov(rotq, HEAD_DIM)
    bad, worst = 0, 0
    for k in full:
        a, b = full[k].astype(np.float64), ours[k].astype(np.float64)
        diff = full[k].view(np.uint16) != ours[k].view(np.uint16)
        bad += int(diff.sum())
        if diff.any():
            ulp = np.spacing(np.maximum(np.abs(full[k]), np.abs(ours[k])).astype(np.float16)).astype(np.float64)
            worst = max(worst, int(np.ceil((np.abs(a - b) / ulp)[diff].max())))
    out["standin_mismatches"], out["standin_max_ulp"] = np.int64(bad), np.int64(worst)

    # n = 128: the divisor is not a power of two, so the reference's matmul rounds per product
    torch.manual_seed(128)
    Q128 = rotation.get_orthogonal_matrix(128, "hadamard", torch.device("cpu"))
    rng = np.random.Generator(np.random.PCG64(128))
    W128 = rng.standard_normal((32, 128)).astype(np.float16)
    emb = torch.nn.Module()
    emb.model = torch.nn.Module()
    emb.model.embed_tokens = torch.nn.Embedding(32, 128).half()
    emb.model.embed_tokens.weight.data = torch.from_numpy(W128.copy())
    with torch.inference_mode():
        rotation.rotate_embeddings(emb, Q128, "qwen2", "cpu")
    out["had128/W"], out["had128/Q"] = W128, Q128.numpy()
    out["had128/signs"] = np.sign(Q128[:, 0].numpy()).astype(np.int8)
    out["had128/out"] = emb.model.embed_tokens.weight.data.numpy().copy()

    path = os.path.join(HERE, "rotate_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", len(out), "arrays; stand-in mismatches", bad, "worst ulp", worst)


if __name__ == "__main__":
    main()
