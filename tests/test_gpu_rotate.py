"""The Hadamard op and the rotation flow on the GPU against the CPU restatement tests/rotate_ref.py, bit for bit: every block size class
(registers only, one trip through LDS, several, the overlapping last trip, 512- and 1024-thread tiles), both dtypes, views inside wider
matrices, in place, crafted rows, block and row independence, graph replay; rotate_model on the fixture model; and quantize_model with
rotation= as the composition of rotate_model and today's flow."""
import copy
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rotate_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 16, 64, 128, 1024, 8192]
NP = {torch.float16: np.float16, torch.float32: np.float32}


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


def _gpu(x, n, sign=None, **kw):
    from qqq_amd.quant import ops

    dev = torch.device("cuda:0")
    y = ops.hadamard_rows(torch.from_numpy(x).to(dev), n, sign=None if sign is None else torch.from_numpy(sign).to(dev), **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_op_is_the_restatement_bit_for_bit(n, dtype):
    for rows in (1, 5, 67):
        for cols in (n, 3 * n):
            x = _rows(n + rows, rows, cols, dtype)
            for sign in (None, _signs(n, n)):
                assert _same(_gpu(x, n, sign), R.hadamard_rows(x, n, sign)), (rows, cols, sign is not None)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_views_padding_and_in_place(dev, n, dtype):
    """x and out inside wider matrices whose padding holds NaN: at a 16-byte aligned offset with a stride that keeps every run aligned
    (the 16-byte loads) and at an odd offset and stride (element by element) -- the same bits; the padding stays; then in place"""
    from qqq_amd.quant import ops

    rows, cols = 5, 3 * n
    x = _rows(7 * n, rows, cols, dtype)
    sign = _signs(n + 1, n)
    want = R.hadamard_rows(x, n, sign)
    sd = torch.from_numpy(sign).to(dev)
    for off, extra in ((8, 16), (3, 7), (0, 1)):
        X = torch.full((rows, cols + off + extra), float("nan"), dtype=dtype, device=dev)
        Y = torch.full((rows, cols + off + extra + 8), float("nan"), dtype=dtype, device=dev)
        X[:, off:off + cols] = torch.from_numpy(x).to(dev)
        xin = X.clone()
        got = ops.hadamard_rows(X[:, off:off + cols], n, sign=sd, out=Y[:, off:off + cols])
        torch.cuda.synchronize()
        assert got.data_ptr() == Y[:, off:off + cols].data_ptr()
        assert _same(got.cpu().numpy(), want), (off, extra)
        assert torch.isnan(Y[:, :off]).all() and torch.isnan(Y[:, off + cols:]).all()  # the padding is not touched
        assert torch.equal(X.view(torch.int16 if dtype == torch.float16 else torch.int32), xin.view(torch.int16 if dtype == torch.float16 else torch.int32))
        # in place, same view
        ops.hadamard_rows(X[:, off:off + cols], n, sign=sd, out=X[:, off:off + cols])
        torch.cuda.synchronize()
        assert _same(X[:, off:off + cols].cpu().numpy(), want), (off, extra, "in place")
        assert torch.isnan(X[:, :off]).all() and torch.isnan(X[:, off + cols:]).all()
    # a sign vector that is a view at an odd offset (no 8-byte load of the signs): the same bits
    held = torch.zeros(n + 3, dtype=torch.int8, device=dev)
    held[3:] = sd
    got = ops.hadamard_rows(torch.from_numpy(x).to(dev), n, sign=held[3:])
    torch.cuda.synchronize()
    assert _same(got.cpu().numpy(), want)


@pytest.mark.parametrize("n", [16, 128, 1024, 8192])
def test_a_blocks_bits_do_not_know_its_place(n):
    """a block alone in a one-row launch, and the same block as block 2 of row 40 of a 67-row launch"""
    for dtype in (torch.float32, torch.float16):
        big = _rows(3 * n, 67, 3 * n, dtype)
        sign = _signs(n + 2, n)
        alone = _gpu(np.ascontiguousarray(big[40:41, 2 * n:3 * n]), n, sign)
        assert _same(_gpu(big, n, sign)[40:41, 2 * n:3 * n], alone)
        other = _rows(5 * n, 67, 3 * n, dtype)
        other[40, 2 * n:3 * n] = big[40, 2 * n:3 * n]
        assert _same(_gpu(other, n, sign)[40:41, 2 * n:3 * n], alone)


def test_crafted_rows():
    # the largest fp16 in every place: exact sums up to 8192 * 65504 < 2^29; what does not fit fp16 becomes inf as torch's cast does
    for n in (16, 8192):
        x = np.full((2, n), 65504.0, np.float16)
        x[1, 1::2] = -65504.0
        want = R.hadamard_rows(x, n)
        assert np.isinf(want[0, 0]) and want[0, 1] == 0 and want[1, 0] == 0 and np.isinf(want[1, 1])
        assert _same(_gpu(x, n), want)
        xf = x.astype(np.float32)  # f32: 8192 * 65504 / sqrt(8192) is finite
        assert np.isfinite(R.hadamard_rows(xf, n)).all() and _same(_gpu(xf, n), R.hadamard_rows(xf, n))
    # fp16 subnormals in, subnormals and zeros out
    rng = np.random.Generator(np.random.PCG64(9))
    sub = (rng.integers(-1023, 1024, size=(3, 256)).astype(np.float64) * 2.0 ** -24).astype(np.float16)
    for n in (4, 64, 256):
        want = R.hadamard_rows(sub, n)
        assert (np.abs(want[want != 0]) < 2.0 ** -14).any()
        assert _same(_gpu(sub, n), want)
    # f32 subnormals survive the round trip through f64
    tiny = (rng.integers(-1000, 1000, size=(2, 64)).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    assert _same(_gpu(tiny, 4), R.hadamard_rows(tiny, 4))
    # the value that exposes f64 -> f32 -> fp16: (d + 2^-11 d + 2^-25 d) / d is a tie only after the f32 rounding
    for n, d in ((4, 2.0), (64, 8.0), (1024, 32.0)):
        x = np.zeros((1, n), np.float16)
        x[0, :3] = [d, d * 2.0 ** -11, d * 2.0 ** -25]
        assert x[0, 2] > 0
        got = _gpu(x, n)
        assert got[0, 0] == np.float16(1.0) and _same(got, R.hadamard_rows(x, n))
        assert np.float64(1 + 2.0 ** -11 + 2.0 ** -25).astype(np.float16) != np.float16(1.0)  # one rounding would go up


def test_replays_from_a_captured_graph(dev):
    from qqq_amd.quant import ops

    n, rows, cols = 1024, 5, 3072
    sign = _signs(77, n)
    sd = torch.from_numpy(sign).to(dev)
    X = torch.zeros((rows, cols), dtype=torch.float16, device=dev)
    Y = torch.zeros_like(X)
    ops.hadamard_rows(X, n, sign=sd, out=Y)  # warm-up outside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.hadamard_rows(X, n, sign=sd, out=Y)
    for seed in (1, 2):
        x = _rows(seed, rows, cols, torch.float16)
        X.copy_(torch.from_numpy(x))
        Y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert _same(Y.cpu().numpy(), R.hadamard_rows(x, n, sign))


CONFIG_FIXTURE = dict(model_type="qwen2", vocab_size=96, hidden_size=64, num_attention_heads=4, num_key_value_heads=2, intermediate_size=128,
                      num_hidden_layers=2, rms_norm_eps=1e-6, rope_theta=10000.0)


def test_rotate_model_on_the_fixture_is_the_restatement(dev):
    from qqq_amd.quant import hadamard_matrix, rotate_model, rotate_state_dict

    g = np.load(os.path.join(ROOT, "tests", "golden", "rotate_small.npz"))
    orig = {k[5:]: g[k] for k in g.files if k.startswith("orig/")}
    signs = g["signs"]
    cfg = SimpleNamespace(**CONFIG_FIXTURE)
    for tied in (True, False):
        src = {k: v for k, v in orig.items() if not (tied and k == "lm_head.weight")}
        want = R.rotate_model(src, 64, 16, signs, tied=tied)
        sd = {k: torch.from_numpy(v.copy()) for k, v in src.items()}
        got, used = rotate_model(sd, cfg, signs=torch.from_numpy(signs.copy()), device=dev)
        assert torch.equal(used, torch.from_numpy(signs)) and sorted(got) == sorted(want)
        for k, v in want.items():
            assert got[k].device.type == "cpu" and _same(got[k].numpy(), v), (tied, k)
        assert all(torch.equal(sd[k], torch.from_numpy(src[k])) for k in src)  # the input is left alone
    # the reference's own Q stage, straight from the fixture (v_proj and o_proj went on through the per-head stage)
    for k in g.files:
        if k.startswith("rotq/") and "v_proj" not in k and "o_proj" not in k:
            assert _same(got[k[5:]].numpy(), g[k]), k
    # f32 state dicts take the same path
    want32 = R.rotate_model({k: v.astype(np.float32) for k, v in orig.items()}, 64, 16, signs)
    got32, _ = rotate_model({k: torch.from_numpy(v.astype(np.float32)) for k, v in orig.items()}, cfg, signs=torch.from_numpy(signs.copy()), device=dev)
    for k, v in want32.items():
        assert _same(got32[k].numpy(), v), k
    # drawn signs: seeded, returned, and the rotation they stand for
    a, sa = rotate_model(sd, cfg, generator=torch.Generator().manual_seed(3), device=dev)
    b, sb = rotate_model(sd, cfg, generator=torch.Generator().manual_seed(3), device=dev)
    assert sa.dtype == torch.int8 and torch.equal(sa, sb) and all(torch.equal(a[k], b[k]) for k in a)
    # the dense branch: an explicit Q that IS the Hadamard matrix gives the kernel path's bits at hidden 64 (exact sums, d = 8);
    # mode="random" returns an orthogonal Q and is the reference's line
    fused = {k: torch.from_numpy(v) for k, v in R.fuse_layer_norms(orig).items()}
    dense, Q = rotate_state_dict(fused, cfg, Q=hadamard_matrix(torch.from_numpy(signs.copy())), device=dev)
    want = R.rotate_model(orig, 64, 16, signs)
    for k, v in want.items():
        assert _same(dense[k].numpy(), v), k
    rnd, Qr = rotate_state_dict(fused, cfg, mode="random", generator=torch.Generator().manual_seed(4), device=dev)
    assert Qr.dtype == torch.float64 and torch.allclose(Qr @ Qr.T, torch.eye(64, dtype=torch.float64), atol=1e-12)
    k = "model.layers.1.mlp.down_proj.weight"
    assert torch.equal(rnd[k], (Qr.to(dev).T @ fused[k].to(dev).double()).half().cpu())
    assert torch.allclose(rnd[k].double(), Qr.T @ fused[k].double(), atol=2e-3, rtol=2e-3)
    k = "model.layers.1.self_attn.q_proj.weight"
    assert torch.equal(rnd[k], (fused[k].to(dev).double() @ Qr.to(dev)).half().cpu())
    assert torch.allclose(rnd[k].double(), fused[k].double() @ Qr, atol=2e-3, rtol=2e-3)


CONFIG = dict(model_type="llama", vocab_size=1000, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
              num_hidden_layers=2, rms_norm_eps=1e-6, rope_theta=10000.0)


def _tiny_model(seed=21):
    """the random 2-layer model of tests/test_gpu_gptq_model.py and 16 x 128 calibration token ids"""
    g = torch.Generator().manual_seed(seed)
    h, inter, v, kv = 256, 512, 1000, 128
    sd = {"model.embed_tokens.weight": torch.randn((v, h), generator=g).half(), "model.norm.weight": (1 + 0.1 * torch.randn(h, generator=g)).half(),
          "lm_head.weight": (0.2 * torch.randn((v, h), generator=g)).half()}
    shapes = {"self_attn.q_proj": (h, h), "self_attn.k_proj": (kv, h), "self_attn.v_proj": (kv, h), "self_attn.o_proj": (h, h),
              "mlp.gate_proj": (inter, h), "mlp.up_proj": (inter, h), "mlp.down_proj": (h, inter)}
    for i in range(2):
        for name, (n, k) in shapes.items():
            sd[f"model.layers.{i}.{name}.weight"] = (torch.randn((n, k), generator=g) * k ** -0.5).half()
        for name in ("input_layernorm", "post_attention_layernorm"):
            sd[f"model.layers.{i}.{name}.weight"] = (1 + 0.1 * torch.randn(h, generator=g)).half()
    return sd, torch.randint(0, v, (16, 128), generator=g)


def test_quantize_model_with_rotation_is_the_composition(dev):
    from qqq_amd import QuantLlamaForCausalLM
    from qqq_amd.quant import quantize_model, rotate_model

    sd, ids = _tiny_model()
    cfg = SimpleNamespace(**CONFIG)
    results = {}
    lm = quantize_model(sd, cfg, ids, 128, mse=True, device=dev, results=results, rotation="hadamard")
    signs = results.pop("rotation")
    assert signs.dtype == torch.int8 and signs.shape == (256,) and len(results) == 14
    assert not hasattr(cfg, "tie_word_embeddings")  # the caller's config is left alone
    untied = SimpleNamespace(**dict(CONFIG, tie_word_embeddings=False))
    fresh = QuantLlamaForCausalLM.from_config(untied, 128)
    fresh.load_state_dict({k: v.cpu() for k, v in lm.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    norms = [k for k in fresh.state_dict() if k.endswith("norm.weight")]
    assert len(norms) == 5 and all(bool((fresh.state_dict()[k] == 1).all()) for k in norms)
    # the flag is only the composition: quantising the pre-rotated state dict gives the same checkpoint and the same greedy tokens
    rotated, used = rotate_model(sd, cfg, signs=signs, device=dev)
    assert torch.equal(used, signs)
    again = quantize_model(rotated, untied, ids, 128, mse=True, device=dev)
    mine, theirs = lm.state_dict(), again.state_dict()
    assert sorted(mine) == sorted(theirs) and all(torch.equal(mine[k], theirs[k]) for k in mine)
    prompts = [ids[0, :5].tolist(), ids[1, :17].tolist()]
    toks = fresh.generate(prompts, 6)
    assert toks == again.generate(prompts, 6) == lm.generate(prompts, 6)
    assert all(len(t) == 6 and all(0 <= x < 1000 for x in t) for t in toks)
    # a tied model comes out untied, and a sign vector or a Q may be given
    tied_cfg = SimpleNamespace(**dict(CONFIG, tie_word_embeddings=True))
    tied_sd = {k: v for k, v in sd.items() if k != "lm_head.weight"}
    res = {}
    t = quantize_model(tied_sd, tied_cfg, ids[:4], -1, device=dev, results=res, rotation=signs)
    assert torch.equal(res["rotation"], signs) and t.lm_head.weight.data_ptr() != t.model.embed_tokens.weight.data_ptr()
    assert tied_cfg.tie_word_embeddings is True
    want, _ = rotate_model(tied_sd, tied_cfg, signs=signs, device=dev)
    assert torch.equal(t.lm_head.weight.cpu(), want["lm_head.weight"]) and torch.equal(t.model.embed_tokens.weight.cpu(), want["model.embed_tokens.weight"])


def test_rotation_none_is_todays_flow(dev):
    from qqq_amd.quant import quantize_model

    sd, ids = _tiny_model()
    tied_cfg = SimpleNamespace(**dict(CONFIG, tie_word_embeddings=True))
    tied_sd = {k: v for k, v in sd.items() if k != "lm_head.weight"}
    for src, cfg in ((sd, SimpleNamespace(**CONFIG)), (tied_sd, tied_cfg)):
        res_a, res_b = {}, {}
        a = quantize_model(src, cfg, ids[:4], 128, device=dev, results=res_a)
        b = quantize_model(src, copy.copy(cfg), ids[:4], 128, device=dev, results=res_b, rotation=None)
        assert "rotation" not in res_b and sorted(res_a) == sorted(res_b)
        sa, sb = a.state_dict(), b.state_dict()
        assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
        # nothing was fused or turned: the norms and the embedding are the input's
        assert torch.equal(sb["model.norm.weight"].cpu(), src["model.norm.weight"])
        assert torch.equal(sb["model.embed_tokens.weight"].cpu(), src["model.embed_tokens.weight"])
    assert b.lm_head.weight.data_ptr() == b.model.embed_tokens.weight.data_ptr()  # the tied model stays tied


def test_command_line_tool_rotates(dev, tmp_path):
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
                        str(tmp_path / "q"), "--rotation", "hadamard", "--rotation-seed", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--mse" in r.stderr  # the hint: the reference pairs rotation with the scale search
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["rotation"] == "hadamard" and line["linears"] == 14 and line["nsamples"] == 4
    assert json.load(open(tmp_path / "q" / "quant_config.json")) == {"group_size": 128, "wbits": 4, "rotation": "hadamard", "rotation_seed": 5}
    saved_cfg = json.load(open(tmp_path / "q" / "config.json"))
    assert saved_cfg == dict(cfg, tie_word_embeddings=False)
    saved = torch.load(tmp_path / "q" / "model.pt", map_location="cpu", weights_only=True)
    fresh = QuantLlamaForCausalLM.from_config(SimpleNamespace(**saved_cfg), 128)
    fresh.load_state_dict(saved, strict=True)
    # the seed is the rotation: the same signs through the library give the same checkpoint
    signs = hadamard_signs(256, torch.Generator().manual_seed(5))
    mine = quantize_model(tied, SimpleNamespace(**cfg), ids[:4], 128, device=dev, rotation=signs).state_dict()
    assert sorted(mine) == sorted(saved) and all(torch.equal(mine[k].cpu(), saved[k]) for k in saved)
