"""ops.upper_factor on the GPU -- the upper factor U of H^-1 by one reverse Cholesky factorisation and one triangular inverse -- against
torch's three-step chain in f64 on the CPU, with the f32 chain's own error on the same matrix as the bound; its layouts, graph replay,
failed pivots and refusals; and gptq_quantize / quantize_model with factor="fused"."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def chain(H):
    return torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(H)), upper=True)


def hessian(n, kind, seed=0):
    """2 / s X^T X in f32, damped as gptq._upper_factor damps it.  plain: s = 4 n samples.  correlated: s = n / 4 samples of
    X G / sqrt(n) + 3 b (b one column per sample), rank-deficient before the damping"""
    g = torch.Generator().manual_seed(1000 * seed + n)
    s = 4 * n if kind == "plain" else n // 4
    X = torch.randn(s, n, generator=g)
    if kind == "correlated":
        X = X @ torch.randn(n, n, generator=g) / n ** 0.5 + 3 * torch.randn(s, 1, generator=g)
    H = (2 / s) * (X.t() @ X)
    H[range(n), range(n)] += 0.01 * torch.mean(torch.diag(H))
    return H


def rel(A, ref):
    return float((torch.triu(A).double() - ref).norm() / ref.norm())


@pytest.mark.parametrize("kind", ["plain", "correlated"])
@pytest.mark.parametrize("n", [64, 128, 192, 320, 640])
def test_against_the_f64_chain(dev, n, kind):
    """relative Frobenius error over the upper triangle against chain(H.double()), at most twice the f32 chain's own on the same H.
    Measured on an MI355X, error / the f32 chain's error, plain | correlated: n = 64 1.17 | 0.80, 128 1.21 | 0.84, 192 1.19 | 1.22,
    320 1.29 | 0.84, 640 1.33 | 0.58"""
    from qqq_amd.quant import ops

    H = hessian(n, kind)
    ref = chain(H.double())
    bound = rel(chain(H), ref)
    U = ops.upper_factor(H.to(dev)).cpu()
    print(f"n {n} {kind}: error {rel(U, ref):.3e}, the f32 chain's {bound:.3e}, ratio {rel(U, ref) / bound:.3f}")
    assert rel(U, ref) <= 2 * bound
    assert not torch.tril(U, -1).any() and bool((torch.diag(U) > 0).all())


def test_the_defining_identity(dev):
    """|| U H U^T - I ||_F in f64 at most twice that of the f32 chain's U (n = 320, correlated)"""
    from qqq_amd.quant import ops

    H = hessian(320, "correlated")
    res = lambda U: float((U.double() @ H.double() @ U.double().t() - torch.eye(320, dtype=torch.float64)).norm())
    got, base = res(ops.upper_factor(H.to(dev)).cpu()), res(chain(H))
    print(f"residual {got:.3e}, the f32 chain's {base:.3e}")
    assert got <= 2 * base


def test_layout_and_graph_replay(dev):
    from qqq_amd.quant import ops

    n = 192
    H, H2 = hessian(n, "correlated").to(dev), hessian(n, "plain", seed=1).to(dev)
    want = ops.upper_factor(H)
    assert torch.equal(want, ops.upper_factor(H))  # two eager calls
    hbuf = torch.full((n + 2, n + 72), 3.0, device=dev)
    ubuf = torch.full((n + 3, n + 12), 5.0, device=dev)
    hv, uv = hbuf[1:n + 1, 8:n + 8], ubuf[2:n + 2, 4:n + 4]
    hv.copy_(H)
    before = hbuf.clone()
    assert ops.upper_factor(hv, out=uv) is uv
    assert torch.equal(uv.view(torch.int32), want.view(torch.int32)) and torch.equal(hbuf, before)  # the contiguous bits; H unchanged
    uv.fill_(5.0)
    assert bool((ubuf == 5.0).all())  # nothing outside the view moved
    # a graph captured on one matrix, replayed on another: the eager bits, every time
    hs, us = H.clone(), torch.empty_like(H)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.upper_factor(hs, out=us, check=False)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, info = ops.upper_factor(hs, out=us, check=False)
    hs.copy_(H2)
    want2 = ops.upper_factor(H2)
    for _ in range(3):
        us.zero_()
        graph.replay()
        assert torch.equal(us.view(torch.int32), want2.view(torch.int32)) and int(info) == 0


@pytest.mark.parametrize("poison", ["negative", "nan"])
def test_not_positive_definite(dev, poison):
    from qqq_amd.quant import ops

    H = hessian(192, "plain")
    if poison == "negative":
        H[70, 70] = -1  # the pivots are taken from the end: 191 ... 71 pass
    else:
        H[5, 100] = float("nan")
    with pytest.raises(RuntimeError, match=r"upper_factor: the matrix is not positive-definite \(pivot \d+\)") as e:
        ops.upper_factor(H.to(dev))
    U, info = ops.upper_factor(H.to(dev), check=False)
    torch.cuda.synchronize()
    assert int(info) > 0 and f"(pivot {int(info)})" in str(e.value) and U.shape == (192, 192)
    assert poison == "nan" or int(info) >= 71


def test_every_argument_rejection(dev):
    from qqq_amd.quant import _lib, ops

    f = ops.upper_factor
    H = torch.zeros((128, 128), device=dev)
    wide = torch.zeros((128, 264), device=dev)
    bad = [
        (lambda: f(H.double()), "upper_factor: H must be a float32 matrix"),
        (lambda: f(H[0]), "upper_factor: H must be a float32 matrix"),
        (lambda: f(H[:64]), "upper_factor: H has the shape"),
        (lambda: f(torch.zeros((96, 96), device=dev)), "no multiple of 64 in 64 ... 32768"),
        (lambda: f(wide.t()[:128, :128]), "upper_factor: H must have unit column stride"),
        (lambda: f(torch.zeros((128, 130), device=dev)[:, :128]), "a multiple of 4, got strides"),
        (lambda: f(wide[:, 2:130]), "upper_factor: H must be 16-byte aligned"),
        (lambda: f(H, out=torch.zeros((64, 64), device=dev)), "upper_factor: out has the shape"),
        (lambda: f(H, out=H.half()), "upper_factor: out must be a float32 matrix"),
        (lambda: f(H.cpu()), "every tensor must be on the GPU"),
        (lambda: f(wide[:, :128], out=wide[:, 64:192]), "qqq_upper_factor: H, U, work and info overlap"),
    ]
    for call, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            call()
    # the entry point itself: n, strides below n, alignment, the workspace inside H
    L, p = _lib.lib(), H.data_ptr()
    u, w, i = wide.data_ptr(), torch.zeros(128 * 256, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    for args, msg in [((p, 128, u, 264, 96, w.data_ptr(), i.data_ptr()), "qqq_upper_factor: n=96 is not a multiple of 64"),
                      ((p, 64, u, 264, 128, w.data_ptr(), i.data_ptr()), "qqq_upper_factor: bad strides"),
                      ((p, 128, u + 4, 264, 128, w.data_ptr(), i.data_ptr()), "qqq_upper_factor: bad argument"),
                      ((p, 128, u, 264, 128, p, i.data_ptr()), "qqq_upper_factor: H, U, work and info overlap")]:
        assert L.qqq_upper_factor(*args, 0, None) == _lib.ERR_ARG and _lib.last_error().startswith(msg)
    torch.cuda.synchronize()
    assert not H.any() and not wide.any() and not w.any() and not i.any()  # nothing was launched


def flow_inputs():
    """the fp16 200 x 384 weight and the Hessian of 512 correlated calibration rows, one column dead, of the flow test of the sweep"""
    rng = np.random.Generator(np.random.PCG64(11))
    W = (rng.standard_normal((200, 384)) * 0.02).astype(np.float16)
    mix = rng.standard_normal((384, 384)) * (rng.random((384, 384)) < 0.05) + np.eye(384)
    X = (rng.standard_normal((512, 384)) * (0.2 + rng.random(384) * 2)) @ mix
    X[:, 77] = 0
    return torch.from_numpy(W), torch.from_numpy((2.0 / 4 * X.T @ X).astype(np.float32))


@pytest.mark.parametrize("gs", [-1, 128])
def test_gptq_quantize_over_the_fused_factor(dev, gs):
    from qqq_amd.quant import gptq_quantize, ops, round_to_nearest

    W, H = (t.to(dev) for t in flow_inputs())
    res = gptq_quantize(W, H, gs, trace=True, factor="fused")
    damped = H.clone()
    damped[77, 77] = 1
    damped[range(384), range(384)] += 0.01 * torch.mean(torch.diag(damped))
    assert torch.equal(res.Hinv.view(torch.int32), ops.upper_factor(damped).view(torch.int32))
    for b in res.trace:
        Q1, Err1 = ops.gptq_block(b.block_in, res.Hinv[b.start:b.start + 128, b.start:b.start + 128], b.scale, gs != -1)
        assert torch.equal(Q1.view(torch.int32), b.Q1.view(torch.int32)) and torch.equal(Err1.view(torch.int32), b.Err1.view(torch.int32))
    Wz = W.double()
    Wz[:, 77] = 0
    loss = lambda Q: float(torch.einsum("ik,kl,il->", Wz - Q.double(), H.double(), Wz - Q.double()))
    got, base = loss(res.weight), loss(round_to_nearest(Wz.half(), res.scales, gs != -1).weight)
    print(f"gs {gs}: proxy loss {got:.4f} = {got / base:.4f} x round-to-nearest")
    assert got < base
    # the default is the parent's chain, bit for bit
    old, same = gptq_quantize(W, H, gs, trace=True), gptq_quantize(W, H, gs, trace=True, factor="torch")
    assert torch.equal(old.Hinv.view(torch.int32), chain(damped).contiguous().view(torch.int32))
    assert torch.equal(old.Hinv.view(torch.int32), same.Hinv.view(torch.int32)) and torch.equal(old.weight, same.weight)
    with pytest.raises(RuntimeError, match="gptq_quantize: factor must be one of"):
        gptq_quantize(W, H, gs, factor="lapack")


def test_quantize_model_over_the_fused_factor(dev):
    from test_gpu_gptq_model import CONFIG, LAYERS, LINEARS, make_state_dict

    from qqq_amd import QuantLlamaForCausalLM, pack
    from qqq_amd.quant import quantize_model

    sd, ids = make_state_dict()
    results = {}
    lm = quantize_model(sd, SimpleNamespace(**CONFIG), ids, 128, device=dev, results=results, factor="fused")
    assert sorted(results) == sorted(f"model.layers.{i}.{n}" for i in range(LAYERS) for n in LINEARS)
    mods = dict(lm.named_modules())
    for name, res in results.items():
        assert torch.equal(pack.unpack_codes(mods[name].B, True).t().to(torch.int8), res.codes()), name
    fresh = QuantLlamaForCausalLM.from_config(SimpleNamespace(**CONFIG), 128)
    fresh.load_state_dict({k: v.cpu() for k, v in lm.state_dict().items()}, strict=True)
    prompt = [ids[0, :5].tolist()]
    assert fresh.to(dev).eval().generate(prompt, 4) == lm.generate(prompt, 4)
