"""ops.hessian_update on the GPU -- GPTQ's Hessian accumulation as one symmetric rank-k launch on the fp16 matrix path -- through
Hessian(accumulate="fused") against the f64 statement H <- H n / (n + b) + (2 / (n + b)) X^T X: exactly where every partial sum is an
integer, and within the f32 add_batch's own error elsewhere; its layouts, graph replay and refusals; and quantize_model(hessian="fused")."""
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu


def statement(calls):
    """the f64 Hessian of the batches `calls` (2-D: one sample, 3-D: its leading dimension)"""
    n = calls[0].shape[-1]
    H, ns = torch.zeros((n, n), dtype=torch.float64), 0
    for x in calls:
        b = 1 if x.dim() == 2 else x.shape[0]
        x = x.double().reshape(-1, n)
        H = H * (ns / (ns + b)) + (2 / (ns + b)) * (x.t() @ x)
        ns += b
    return H


def accumulated(calls, device, accumulate):
    from qqq_amd.quant import Hessian

    h = Hessian(calls[0].shape[-1], device, accumulate)
    for x in calls:
        h.add_batch(x.to(device))
    return h


@pytest.mark.parametrize("shapes", [[(1,)], [(200,), (1, 63), (2, 100)]], ids=["one_token", "three_calls"])
@pytest.mark.parametrize("n", [64, 192, 320])
def test_exact_on_small_integers(dev, n, shapes):
    """integers -3 ... 3 and sample counts 1, 2, 4: every product, partial sum, alpha and beta is exact in f32, so H equals the f64
    statement element for element; it equals its transpose, and a dead column's row and column are exact zeros"""
    g = torch.Generator().manual_seed(n)
    calls = [torch.randint(-3, 4, (*s, n), generator=g).half() for s in shapes]
    for x in calls:
        x[..., n - 3] = 0
    h = accumulated(calls, dev, "fused")
    H = h.H.cpu()
    assert h.nsamples == sum(1 if x.dim() == 2 else x.shape[0] for x in calls)
    assert torch.equal(H.double(), statement(calls)) and torch.equal(H, H.t())
    assert not H[n - 3].any() and not H[:, n - 3].any() and bool((torch.diag(H)[:n - 3] > 0).any())


@pytest.mark.parametrize("kind", ["plain", "correlated"])
@pytest.mark.parametrize("n", [192, 320])
def test_against_f64_on_real_inputs(dev, n, kind):
    """relative Frobenius error against the f64 statement, at most twice that of the unchanged f32 add_batch on the same fp16 inputs
    (three calls of [2, 200, n]).  Measured on an MI355X, error / the f32 path's error, plain | correlated: n = 192 0.73 | 0.56,
    320 0.68 | 0.54"""
    g = torch.Generator().manual_seed(7 * n)
    calls = []
    for _ in range(3):
        x = torch.randn(2, 200, n, generator=g)
        if kind == "correlated":
            x = x * (0.2 + 2 * torch.rand(n, generator=g)) + 3 * torch.randn(2, 200, 1, generator=g)
        calls.append(x.half())
    ref = statement(calls)
    rel = lambda H: float((H.double() - ref).norm() / ref.norm())
    bound = rel(accumulated(calls, "cpu", "torch").H)
    got = rel(accumulated(calls, dev, "fused").H.cpu())
    print(f"n {n} {kind}: error {got:.3e}, the f32 add_batch's {bound:.3e}, ratio {got / bound:.3f}")
    assert got <= 2 * bound


def test_layout_nan_and_graph_replay(dev):
    from qqq_amd.quant import ops

    n, g = 192, torch.Generator().manual_seed(3)
    x, x2 = (torch.randn(150, n, generator=g).half().to(dev) for _ in range(2))
    H0 = torch.randn(n, n, generator=g).to(dev)
    want = ops.hessian_update(H0.clone(), x, 0.75, 0.5)
    hbuf = torch.full((n + 2, n + 72), 3.0, device=dev)
    xbuf = torch.full((152, n + 24), 5.0, dtype=torch.float16, device=dev)
    hv, xv = hbuf[1:n + 1, 8:n + 8], xbuf[1:151, 8:n + 8]
    hv.copy_(H0)
    xv.copy_(x)
    xkeep = xbuf.clone()
    assert ops.hessian_update(hv, xv, 0.75, 0.5) is hv
    assert torch.equal(hv.view(torch.int32), want.view(torch.int32)) and torch.equal(xbuf, xkeep)  # the contiguous bits; X unchanged
    hv.fill_(3.0)
    assert bool((hbuf == 3.0).all())  # nothing outside the view moved
    # alpha == 0 does not read H
    clean = ops.hessian_update(torch.zeros((n, n), device=dev), x, 0.0, 2.0)
    assert torch.equal(ops.hessian_update(torch.full((n, n), float("nan"), device=dev), x, 0.0, 2.0), clean)
    # a graph captured on one X, replayed on another: the eager bits, every time
    hs, xs = H0.clone(), x.clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.hessian_update(hs, xs, 0.75, 0.5)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.hessian_update(hs, xs, 0.75, 0.5)
    xs.copy_(x2)
    want2 = ops.hessian_update(H0.clone(), x2, 0.75, 0.5)
    for _ in range(3):
        hs.copy_(H0)
        graph.replay()
        assert torch.equal(hs.view(torch.int32), want2.view(torch.int32))


def test_every_argument_rejection(dev):
    from qqq_amd.quant import Hessian, _lib, ops

    f = ops.hessian_update
    H, x = torch.zeros((128, 128), device=dev), torch.zeros((8, 128), dtype=torch.float16, device=dev)
    wide = torch.zeros((128, 264), device=dev)
    bad = [
        (lambda: f(H.double(), x, 1, 1), "hessian_update: H must be a float32 matrix"),
        (lambda: f(H[:64], x, 1, 1), "hessian_update: H has the shape"),
        (lambda: f(torch.zeros((96, 96), device=dev), x, 1, 1), "no multiple of 64 in 64 ... 32768"),
        (lambda: f(wide.t()[:128, :128], x, 1, 1), "hessian_update: H must have unit column stride"),
        (lambda: f(wide[:, 2:130], x, 1, 1), "hessian_update: H must be 16-byte aligned"),
        (lambda: f(H, x.float(), 1, 1), "hessian_update: x must be a float16 matrix"),
        (lambda: f(H, x[0], 1, 1), "hessian_update: x must be a float16 matrix"),
        (lambda: f(H, x[:, :64], 1, 1), "hessian_update: x has the shape"),
        (lambda: f(H, x[:0], 1, 1), "hessian_update: x has the shape"),
        (lambda: f(H, x.cpu(), 1, 1), "hessian_update: every tensor must be on the GPU"),
        (lambda: Hessian(128, dev, "lapack"), "Hessian: accumulate must be one of"),
        (lambda: Hessian(128, dev, "fused").add_batch(x.float()), "Hessian.add_batch: accumulate='fused' takes float16 inputs on the GPU"),
        (lambda: Hessian(128, dev, "fused").add_batch(x[:, :64]), "Hessian.add_batch: the input's last dimension is 64"),
    ]
    for call, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            call()
    # the entry point itself: n, tokens, strides, alignment, X inside H
    L, p, q = _lib.lib(), H.data_ptr(), x.data_ptr()
    for args, msg in [((p, 128, q, 128, 8, 96), "qqq_hessian_update: n=96 is not a multiple of 64"),
                      ((p, 128, q, 128, 0, 128), "qqq_hessian_update: tokens=0 must be at least 1"),
                      ((p, 64, q, 128, 8, 128), "qqq_hessian_update: bad strides"),
                      ((p, 128, q, 132, 8, 128), "qqq_hessian_update: bad strides"),
                      ((p, 128, q + 8, 128, 8, 128), "qqq_hessian_update: bad argument"),
                      ((p, 128, p + 256, 128, 8, 128), "qqq_hessian_update: H and X overlap")]:
        assert L.qqq_hessian_update(*args, 1.0, 1.0, 0, None) == _lib.ERR_ARG and _lib.last_error().startswith(msg)
    torch.cuda.synchronize()
    assert not H.any() and not wide.any() and not x.any()  # nothing was launched


def test_quantize_model_over_the_fused_hessian(dev):
    from test_gpu_gptq_model import CONFIG, LAYERS, LINEARS, make_state_dict

    from qqq_amd import QuantLlamaForCausalLM, pack
    from qqq_amd.quant import Hessian, quantize_model

    sd, ids = make_state_dict()
    results = {}
    lm = quantize_model(sd, SimpleNamespace(**CONFIG), ids, 128, device=dev, results=results, hessian="fused")
    assert sorted(results) == sorted(f"model.layers.{i}.{n}" for i in range(LAYERS) for n in LINEARS)
    mods = dict(lm.named_modules())
    for name, res in results.items():
        assert torch.equal(pack.unpack_codes(mods[name].B, True).t().to(torch.int8), res.codes()), name
    fresh = QuantLlamaForCausalLM.from_config(SimpleNamespace(**CONFIG), 128)
    fresh.load_state_dict({k: v.cpu() for k, v in lm.state_dict().items()}, strict=True)
    prompt = [ids[0, :5].tolist()]
    assert fresh.to(dev).eval().generate(prompt, 4) == lm.generate(prompt, 4)
    # "torch" and the default: the parent's add_batch, bit for bit
    x = torch.randn(2, 50, 128, generator=torch.Generator().manual_seed(5)).half().to(dev)
    want, ns = torch.zeros((128, 128), device=dev), 0
    for _ in range(2):
        want *= ns / (ns + 2)
        ns += 2
        xf = math.sqrt(2 / ns) * x.reshape(-1, 128).float()
        want += xf.t().matmul(xf)
    for h in (Hessian(128, dev), Hessian(128, dev, "torch")):
        h.add_batch(x)
        h.add_batch(x)
        assert torch.equal(h.H.view(torch.int32), want.view(torch.int32)) and h.nsamples == 4
