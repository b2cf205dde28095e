"""The Hadamard op for blocks of K * 2^p columns and the rotation mode over it on the GPU, against the CPU restatement
tests/rotate_k_ref.py bit for bit: every layout class (m = 1 with runs of 4 and of 8, m < 8 with several sub-blocks in a run, register
stages only, one and several trips through LDS, blocks that share a workgroup, 512- and 1024-thread workgroups), both dtypes, our tables
and the reference's (recovered from the recorded Q of tests/golden/rotate_k_small.npz), views, misaligned pointers, in place, crafted
rows, graph replay; rotate_model(mode="hadamard_k") on the fixture model against the reference's recorded Q stage; the function of the
rotated model; quantize_model(rotation="hadamard_k") as the composition of rotate_model and the plain flow; the command-line tool."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rotate_k_ref as RK
import rotate_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(12, 1), (12, 2), (12, 4), (12, 8), (20, 1), (28, 4), (28, 32), (40, 4), (12, 128), (28, 128), (40, 128), (28, 256)]
NP = {torch.float16: np.float16, torch.float32: np.float32}
FIXTURE_Q = {12: "had12", 20: "had20", 28: "had112", 40: "had160"}  # where the fixture holds the reference's Q of each order


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _rows(seed, rows, cols, dtype):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((rows, cols)) * np.exp2(rng.integers(-6, 4, size=(rows, 1)))  # rows of different magnitude
    return x.astype(NP[dtype])


def _signs(seed, n):
    return (np.random.Generator(np.random.PCG64(seed)).integers(0, 2, size=n) * 2 - 1).astype(np.int8)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "rotate_k_small.npz"))


@pytest.fixture(scope="module")
def tables(fx):
    """{K: (ours, the reference's recovered from its recorded Q)} as numpy int8"""
    from qqq_amd.quant import hadamard_table

    return {k: (hadamard_table(k).numpy(), RK.recover_table(fx[tag + "/Q"], fx[tag + "/signs"], k)) for k, tag in FIXTURE_Q.items()}


def _gpu(x, m, table, sign=None, **kw):
    from qqq_amd.quant import ops

    dev = torch.device("cuda:0")
    y = ops.hadamard_rows_k(torch.from_numpy(x).to(dev), m, torch.from_numpy(table).to(dev),
                            sign=None if sign is None else torch.from_numpy(sign).to(dev), **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "f32"])
@pytest.mark.parametrize("K,m", SHAPES)
def test_op_is_the_restatement_bit_for_bit(tables, K, m, dtype):
    n = K * m
    for rows in (1, 3, 33):
        x = _rows(n + rows, rows, n * (2 if n <= 1536 else 1), dtype)
        for table in tables[K]:
            for sign in (None, _signs(n, n)):
                assert _same(_gpu(x, m, table, sign), RK.hadamard_rows_k(x, m, table, sign)), (rows, sign is not None)


def test_a_callers_table_of_any_order_up_to_64(dev):
    """orders the library builds no table for: 4, 16 and 64 (Sylvester: the op is then H_n on fp16, exactly), and 24 (the double of ours)"""
    h2 = np.array([[1, 1], [1, -1]], np.int64)
    h4 = np.kron(h2, h2)
    from qqq_amd.quant import check_table, hadamard_table

    t24 = np.kron(h2, hadamard_table(12).numpy().astype(np.int64))
    for table, m in ((h4, 1), (h4, 2), (h4, 512), (h4, 2048), (np.kron(h4, h4), 4), (np.kron(np.kron(h4, h4), h4), 128), (t24, 16)):
        table = np.ascontiguousarray(table.astype(np.int8))
        check_table(torch.from_numpy(table))
        n = table.shape[0] * m
        for dtype in (torch.float16, torch.float32):
            x = _rows(n, 3, n, dtype)
            sign = _signs(n + 1, n)
            got = _gpu(x, m, table, sign)
            assert _same(got, RK.hadamard_rows_k(x, m, table, sign)), (n, dtype)
            if dtype == torch.float16 and table.shape[0] != 24:
                assert _same(got, R.hadamard_rows(x, n, sign)), n  # exact sums: the order of the adds does not show


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "f32"])
@pytest.mark.parametrize("K,m", [(12, 1), (12, 2), (20, 1), (12, 8), (28, 4), (40, 128)])
def test_views_padding_misaligned_pointers_and_in_place(dev, tables, K, m, dtype):
    """x and out inside wider matrices whose padding holds NaN: at a 16-byte aligned offset with a stride that keeps every run aligned
    (the 16-byte loads) and at odd offsets and strides (element by element) -- the same bits; the padding stays; then in place"""
    from qqq_amd.quant import ops

    n = K * m
    rows, cols = 5, 2 * n
    x = _rows(7 * n, rows, cols, dtype)
    sign = _signs(n + 1, n)
    table = tables[K][1]
    want = RK.hadamard_rows_k(x, m, table, sign)
    sd, td = torch.from_numpy(sign).to(dev), torch.from_numpy(table).to(dev)
    view = torch.int16 if dtype == torch.float16 else torch.int32
    for off, extra in ((8, 16), (3, 7), (0, 1), (1, 0)):
        X = torch.full((rows, cols + off + extra), float("nan"), dtype=dtype, device=dev)
        Y = torch.full((rows, cols + off + extra + 8), float("nan"), dtype=dtype, device=dev)
        X[:, off:off + cols] = torch.from_numpy(x).to(dev)
        xin = X.clone()
        got = ops.hadamard_rows_k(X[:, off:off + cols], m, td, sign=sd, out=Y[:, off:off + cols])
        torch.cuda.synchronize()
        assert got.data_ptr() == Y[:, off:off + cols].data_ptr()
        assert _same(got.cpu().numpy(), want), (off, extra)
        assert torch.isnan(Y[:, :off]).all() and torch.isnan(Y[:, off + cols:]).all()  # the padding is not touched
        assert torch.equal(X.view(view), xin.view(view))
        ops.hadamard_rows_k(X[:, off:off + cols], m, td, sign=sd, out=X[:, off:off + cols])  # in place, same view
        torch.cuda.synchronize()
        assert _same(X[:, off:off + cols].cpu().numpy(), want), (off, extra, "in place")
        assert torch.isnan(X[:, :off]).all() and torch.isnan(X[:, off + cols:]).all()
    # a sign vector that is a view at an odd offset (no 8-byte load of the signs), and a table that is one: the same bits
    held = torch.zeros(n + 3, dtype=torch.int8, device=dev)
    held[3:] = sd
    tab = torch.zeros(K * K + 1, dtype=torch.int8, device=dev)
    tab[1:] = td.flatten()
    got = ops.hadamard_rows_k(torch.from_numpy(x).to(dev), m, tab[1:].view(K, K), sign=held[3:])
    torch.cuda.synchronize()
    assert _same(got.cpu().numpy(), want)


@pytest.mark.parametrize("K,m", [(12, 1), (12, 8), (28, 32), (40, 128)])
def test_a_blocks_bits_do_not_know_its_place(tables, K, m):
    """a block alone in a one-row launch, and the same block as block 2 of row 20 of a 33-row launch"""
    n = K * m
    table = tables[K][0]
    for dtype in (torch.float32, torch.float16):
        big = _rows(3 * n, 33, 3 * n, dtype)
        sign = _signs(n + 2, n)
        alone = _gpu(np.ascontiguousarray(big[20:21, 2 * n:3 * n]), m, table, sign)
        assert _same(_gpu(big, m, table, sign)[20:21, 2 * n:3 * n], alone)
        other = _rows(5 * n, 33, 3 * n, dtype)
        other[20, 2 * n:3 * n] = big[20, 2 * n:3 * n]
        assert _same(_gpu(other, m, table, sign)[20:21, 2 * n:3 * n], alone)


def test_crafted_rows(tables):
    # the largest fp16 in every place at n = 7168: partial sums up to 7168 * 65504 < 2^29 stay exact; what does not fit fp16 becomes inf
    K, m = 28, 256
    n = K * m
    for table in tables[K]:
        x = np.full((3, n), 65504.0, np.float16)
        x[1, 1::2] = -65504.0
        x[2] *= np.repeat(table[5], m).astype(np.float16)  # row 5 of the table adds every sub-block up: the full 2^29-sized sum
        want = RK.hadamard_rows_k(x, m, table)
        assert np.isinf(want).any() and (want == 0).any() and np.isinf(want[2, 5 * m])
        assert _same(_gpu(x, m, table), want)
        xf = x.astype(np.float32)  # f32: 7168 * 65504 / sqrt(7168) is finite
        wf = RK.hadamard_rows_k(xf, m, table)
        assert np.isfinite(wf).all() and wf[2, 5 * m] == np.float32(np.float64(n * 65504.0) / R.divisor(n)) and _same(_gpu(xf, m, table), wf)
    # signed zeros: a flip keeps a zero's sign, -0 + -0 = -0, +0 + -0 = +0
    negative = 0
    for K, m in ((12, 1), (12, 4), (40, 4)):
        n = K * m
        for table in tables[K]:
            for dtype in (np.float16, np.float32):
                z = np.zeros((4, n), dtype)
                z[1] = -0.0
                z[2, ::2] = -0.0
                z[3, : n // 2] = -0.0
                for sign in (None, _signs(n, n)):
                    want = RK.hadamard_rows_k(z, m, table, sign)
                    assert (want == 0).all() and not np.signbit(want).all()
                    negative += int(np.signbit(want).sum())
                    assert _same(_gpu(z, m, table, sign), want), (K, m, dtype)
    assert negative > 0  # the cases do produce -0
    # inf and NaN stay in their block: the block beside has the bits it has alone
    for K, m in ((12, 2), (28, 32), (40, 128)):
        n = K * m
        table = tables[K][0]
        for dtype in (torch.float16, torch.float32):
            x = _rows(n, 2, 3 * n, dtype)
            clean = RK.hadamard_rows_k(x, m, table)
            x[0, n + 3] = np.inf  # one inf: every output of the block is +-inf
            x[1, n + 1], x[1, n + n // 2] = np.inf, np.nan
            got = _gpu(x, m, table)
            assert _same(got[:, :n], clean[:, :n]) and _same(got[:, 2 * n:], clean[:, 2 * n:])
            assert np.isinf(got[0, n:2 * n]).all() and np.isnan(got[1, n:2 * n]).all()
            want = RK.hadamard_rows_k(x, m, table)
            assert _same(got[0], want[0])


def test_replays_from_a_captured_graph(dev, tables):
    from qqq_amd.quant import ops

    K, m, rows = 28, 32, 5
    n = K * m
    sign = _signs(77, n)
    sd = torch.from_numpy(sign).to(dev)
    table = tables[K][1]
    td = torch.from_numpy(table).to(dev)
    X = torch.zeros((rows, 2 * n), dtype=torch.float16, device=dev)
    Y = torch.zeros_like(X)
    ops.hadamard_rows_k(X, m, td, sign=sd, out=Y)  # warm-up outside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.hadamard_rows_k(X, m, td, sign=sd, out=Y)
    for seed in (1, 2):
        x = _rows(seed, rows, 2 * n, torch.float16)
        X.copy_(torch.from_numpy(x))
        Y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert _same(Y.cpu().numpy(), RK.hadamard_rows_k(x, m, table, sign))
    # the table is read on the device: other contents, the same graph
    ours = tables[K][0]
    td.copy_(torch.from_numpy(ours))
    g.replay()
    torch.cuda.synchronize()
    assert _same(Y.cpu().numpy(), RK.hadamard_rows_k(x, m, ours, sign))


CONFIG_FIXTURE = dict(model_type="qwen2", vocab_size=48, hidden_size=96, num_attention_heads=6, num_key_value_heads=2, intermediate_size=64,
                      num_hidden_layers=2, rms_norm_eps=1e-6, rope_theta=10000.0)


def _stage(fx, tag):
    return {k[len(tag) + 1:]: fx[k] for k in fx.files if k.startswith(tag + "/")}


def test_rotate_model_on_the_fixture(dev, fx):
    """with the reference's table: the reference's recorded Q stage except at the recorded mismatches (none), and the restatement bit for
    bit; with ours: the restatement bit for bit"""
    from qqq_amd.quant import hadamard_factor, hadamard_table, rotate_model, rotate_state_dict

    orig = _stage(fx, "orig")
    signs = fx["signs"]
    theirs = RK.recover_table(fx["Q"], signs, 12)
    cfg = SimpleNamespace(**CONFIG_FIXTURE)
    assert hadamard_factor(96) == (12, 8)
    for tied in (True, False):
        src = {k: v for k, v in orig.items() if not (tied and k == "lm_head.weight")}
        sd = {k: torch.from_numpy(v.copy()) for k, v in src.items()}
        for table in (theirs, None):
            want = RK.rotate_model(src, 96, 16, signs, hadamard_table(12).numpy() if table is None else table, tied=tied)
            got, used = rotate_model(sd, cfg, mode="hadamard_k", signs=torch.from_numpy(signs.copy()), device=dev,
                                     table=None if table is None else torch.from_numpy(table))
            assert torch.equal(used, torch.from_numpy(signs)) and sorted(got) == sorted(want)
            for k, v in want.items():
                assert got[k].device.type == "cpu" and _same(got[k].numpy(), v), (tied, table is None, k)
            assert all(torch.equal(sd[k], torch.from_numpy(src[k])) for k in src)  # the input is left alone
            if table is not None and not tied:
                bad = 0
                for k in fx.files:  # v_proj and o_proj went on through the per-head stage
                    if k.startswith("rotq/") and "v_proj" not in k and "o_proj" not in k:
                        bad += int((_bits(got[k[5:]].numpy()) != _bits(fx[k])).sum())
                assert bad == int(fx["mismatches/model"])
    # f32 state dicts take the same path
    want32 = RK.rotate_model({k: v.astype(np.float32) for k, v in orig.items()}, 96, 16, signs, theirs)
    got32, _ = rotate_model({k: torch.from_numpy(v.astype(np.float32)) for k, v in orig.items()}, cfg, mode="hadamard_k",
                            signs=torch.from_numpy(signs.copy()), table=torch.from_numpy(theirs), device=dev)
    for k, v in want32.items():
        assert _same(got32[k].numpy(), v), k
    # drawn signs: seeded and returned
    a, sa = rotate_model(sd, cfg, mode="hadamard_k", generator=torch.Generator().manual_seed(3), device=dev)
    b, sb = rotate_model(sd, cfg, mode="hadamard_k", generator=torch.Generator().manual_seed(3), device=dev)
    assert sa.dtype == torch.int8 and sa.shape == (96,) and torch.equal(sa, sb) and all(torch.equal(a[k], b[k]) for k in a)
    # a power-of-two hidden size: the mode is "hadamard"
    g64 = np.load(os.path.join(ROOT, "tests", "golden", "rotate_small.npz"))
    sd64 = {k[5:]: torch.from_numpy(g64[k]) for k in g64.files if k.startswith("orig/")}
    cfg64 = SimpleNamespace(**dict(CONFIG_FIXTURE, vocab_size=96, hidden_size=64, num_attention_heads=4, intermediate_size=128))
    s64 = torch.from_numpy(g64["signs"])
    x, _ = rotate_model(sd64, cfg64, mode="hadamard_k", signs=s64, device=dev)
    y, _ = rotate_model(sd64, cfg64, mode="hadamard", signs=s64, device=dev)
    assert sorted(x) == sorted(y) and all(torch.equal(x[k], y[k]) for k in x)
    # the dense line with the matrix the mode stands for: the same weights up to the rounding of its products
    from qqq_amd.quant import hadamard_matrix_k

    fused = {k: torch.from_numpy(v) for k, v in R.fuse_layer_norms(orig).items()}
    Q = hadamard_matrix_k(torch.from_numpy(signs), torch.from_numpy(theirs), 8)
    dense, _ = rotate_state_dict(fused, cfg, Q=Q, device=dev)
    fast, _ = rotate_state_dict(fused, cfg, mode="hadamard_k", signs=torch.from_numpy(signs.copy()), table=torch.from_numpy(theirs), device=dev)
    for k in dense:
        assert torch.allclose(dense[k].float(), fast[k].float(), atol=2e-3, rtol=2e-3), k


def _logits32(sd, ids, dev):
    """fp32 forward of the float model on the GPU: FloatDecoderLayer per layer, the final norm, the head"""
    from qqq_amd.quant import FloatDecoderLayer
    from qqq_amd.quant.model import _rms_norm

    cfg = SimpleNamespace(**CONFIG_FIXTURE)
    t = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(dev).float() for k, v in sd.items()}
    x = torch.nn.functional.embedding(ids.to(dev), t["model.embed_tokens.weight"])
    for p in R.layer_prefixes(sd):
        x = FloatDecoderLayer(cfg, {k[len(p):]: v for k, v in t.items() if k.startswith(p)}).forward(x)
    x = _rms_norm(x, t["model.norm.weight"], CONFIG_FIXTURE["rms_norm_eps"])
    return (x @ t["lm_head.weight"].t()).double().cpu()


def _logits64(sd, ids):
    from qqq_amd.quant import FloatDecoderLayer
    from qqq_amd.quant.model import _rms_norm

    cfg = SimpleNamespace(**CONFIG_FIXTURE)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in sd.items()}
    x = torch.nn.functional.embedding(ids, t["model.embed_tokens.weight"])
    for p in R.layer_prefixes(sd):
        x = FloatDecoderLayer(cfg, {k[len(p):]: v for k, v in t.items() if k.startswith(p)}).forward(x)
    x = _rms_norm(x, t["model.norm.weight"], CONFIG_FIXTURE["rms_norm_eps"])
    return x @ t["lm_head.weight"].t()


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_rotation_leaves_the_models_function_alone(dev, fx):
    """2 x 16 tokens, fp32 logits on the GPU against an fp64 forward of the UNROTATED model on the CPU.  The yardstick is the deviation
    the REFERENCE's rotated weights show (its recorded Q stage, then the per-head stage) under the same fp32 forward; ours may be twice
    that, the margin of tests/test_rotate_ref_cpu.py: both pipelines round every weight the same number of times."""
    from qqq_amd.quant import rotate_model

    orig = _stage(fx, "orig")
    ids = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).integers(0, 48, size=(2, 16)))
    want = _logits64(orig, ids)
    reference = R.rotate_ov(dict(dict(orig, **_stage(fx, "fused")), **_stage(fx, "rotq")), 16)
    ref_dev = _rel(_logits32(reference, ids, dev), want)
    plain = _rel(_logits32(orig, ids, dev), want)
    cfg = SimpleNamespace(**CONFIG_FIXTURE)
    sd = {k: torch.from_numpy(v.copy()) for k, v in orig.items()}
    for table in (None, torch.from_numpy(RK.recover_table(fx["Q"], fx["signs"], 12))):
        mine, _ = rotate_model(sd, cfg, mode="hadamard_k", signs=torch.from_numpy(fx["signs"].copy()), table=table, device=dev)
        my_dev = _rel(_logits32(mine, ids, dev), want)
        print(f"relative L2 deviation of the logits: fp32 forward alone {plain:.3e}, reference's rotated weights {ref_dev:.3e}, ours {my_dev:.3e}")
        assert plain < ref_dev / 20 and 0 < ref_dev < 1e-2  # fp16 weight rounding, not the forward and not a different function
        assert my_dev <= 2 * ref_dev
        # the stages matter: with one weight of the Q stage left unturned the function is another one
        half = dict(mine)
        half["model.layers.0.mlp.down_proj.weight"] = torch.from_numpy(orig["model.layers.0.mlp.down_proj.weight"])
        assert _rel(_logits32(half, ids, dev), want) > 20 * ref_dev


# QuantLinear admits no 96-wide layer (the reference's shape rule: in-features a multiple of 64, out-features of 64 with 128 in):
# 384 = 12 * 32 is the smallest 12 * 2^p the packed model takes
CONFIG = dict(model_type="llama", vocab_size=512, hidden_size=384, num_attention_heads=6, num_key_value_heads=2, intermediate_size=512,
              num_hidden_layers=2, rms_norm_eps=1e-6, rope_theta=10000.0)


def _tiny_model(seed=22):
    g = torch.Generator().manual_seed(seed)
    h, inter, v, kv = 384, 512, 512, 128
    sd = {"model.embed_tokens.weight": torch.randn((v, h), generator=g).half(), "model.norm.weight": (1 + 0.1 * torch.randn(h, generator=g)).half(),
          "lm_head.weight": (0.2 * torch.randn((v, h), generator=g)).half()}
    shapes = {"self_attn.q_proj": (h, h), "self_attn.k_proj": (kv, h), "self_attn.v_proj": (kv, h), "self_attn.o_proj": (h, h),
              "mlp.gate_proj": (inter, h), "mlp.up_proj": (inter, h), "mlp.down_proj": (h, inter)}
    for i in range(2):
        for name, (n, k) in shapes.items():
            sd[f"model.layers.{i}.{name}.weight"] = (torch.randn((n, k), generator=g) * k ** -0.5).half()
        for name in ("input_layernorm", "post_attention_layernorm"):
            sd[f"model.layers.{i}.{name}.weight"] = (1 + 0.1 * torch.randn(h, generator=g)).half()
    return sd, torch.randint(0, v, (8, 128), generator=g)


def test_quantize_model_with_hadamard_k_is_the_composition(dev):
    from qqq_amd import QuantLlamaForCausalLM
    from qqq_amd.quant import quantize_model, rotate_model

    with pytest.raises(ValueError, match="Not supported `infeatures`: 96"):  # why this test is not at hidden 96
        QuantLlamaForCausalLM.from_config(SimpleNamespace(**dict(CONFIG, hidden_size=96, intermediate_size=128)), 128)
    sd, ids = _tiny_model()
    cfg = SimpleNamespace(**CONFIG)
    results = {}
    lm = quantize_model(sd, cfg, ids, 128, mse=True, device=dev, results=results, rotation="hadamard_k")
    signs = results.pop("rotation")
    assert signs.dtype == torch.int8 and signs.shape == (384,) and len(results) == 14
    assert not hasattr(cfg, "tie_word_embeddings")  # the caller's config is left alone
    untied = SimpleNamespace(**dict(CONFIG, tie_word_embeddings=False))
    norms = [k for k in lm.state_dict() if k.endswith("norm.weight")]
    assert len(norms) == 5 and all(bool((lm.state_dict()[k] == 1).all()) for k in norms)
    # the flag is only the composition: quantising the pre-rotated state dict gives the same checkpoint and the same greedy tokens
    rotated, used = rotate_model(sd, cfg, mode="hadamard_k", signs=signs, device=dev)
    assert torch.equal(used, signs)
    again = quantize_model(rotated, untied, ids, 128, mse=True, device=dev)
    mine, theirs = lm.state_dict(), again.state_dict()
    assert sorted(mine) == sorted(theirs) and all(torch.equal(mine[k], theirs[k]) for k in mine)
    prompts = [ids[0, :5].tolist(), ids[1, :17].tolist()]
    toks = lm.generate(prompts, 6)
    assert toks == again.generate(prompts, 6) and all(len(t) == 6 and all(0 <= x < 512 for x in t) for t in toks)
    # the pair the tool passes: the same signs, the same checkpoint
    res = {}
    pair = quantize_model(sd, cfg, ids, 128, mse=True, device=dev, results=res, rotation=("hadamard_k", signs))
    assert torch.equal(res["rotation"], signs) and all(torch.equal(mine[k], v) for k, v in pair.state_dict().items())
    # mode "hadamard" still refuses the size
    with pytest.raises(RuntimeError, match="rotate_state_dict: hidden_size = 384 is not a power of two.*Paley.*mode='random'"):
        quantize_model(sd, cfg, ids[:1], 128, device=dev, rotation="hadamard")


def test_command_line_tool_rotates_with_hadamard_k(dev, tmp_path):
    from qqq_amd import QuantLlamaForCausalLM
    from qqq_amd.quant import hadamard_signs, quantize_model

    sd, ids = _tiny_model()
    tied = {k: v for k, v in sd.items() if k != "lm_head.weight"}
    cfg = dict(CONFIG, tie_word_embeddings=True)
    json.dump(cfg, open(tmp_path / "config.json", "w"))
    torch.save(tied, tmp_path / "model.pt")
    np.save(tmp_path / "calib.npy", ids[:4].numpy())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "quantize_model.py"), "--config", str(tmp_path / "config.json"), "--weights",
                        str(tmp_path / "model.pt"), "--tokens", str(tmp_path / "calib.npy"), "--group-size", "128", "--seqlen", "128", "--out",
                        str(tmp_path / "q"), "--rotation", "hadamard_k", "--rotation-seed", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["rotation"] == "hadamard_k" and line["linears"] == 14 and line["nsamples"] == 4
    assert json.load(open(tmp_path / "q" / "quant_config.json")) == {"group_size": 128, "wbits": 4, "rotation": "hadamard_k", "rotation_seed": 5}
    saved_cfg = json.load(open(tmp_path / "q" / "config.json"))
    assert saved_cfg == dict(cfg, tie_word_embeddings=False)
    saved = torch.load(tmp_path / "q" / "model.pt", map_location="cpu", weights_only=True)
    fresh = QuantLlamaForCausalLM.from_config(SimpleNamespace(**saved_cfg), 128)
    fresh.load_state_dict(saved, strict=True)
    # the seed is the rotation: the same signs through the library give the same checkpoint
    signs = hadamard_signs(384, torch.Generator().manual_seed(5))
    mine = quantize_model(tied, SimpleNamespace(**cfg), ids[:4], 128, device=dev, rotation=("hadamard_k", signs)).state_dict()
    assert sorted(mine) == sorted(saved) and all(torch.equal(mine[k].cpu(), saved[k]) for k in saved)
