"""ops.hessian_update_grouped on the GPU -- the Hessians of all experts of a mixture-of-experts layer in one launch that gathers its rows
through the routing -- against the f64 statement per expert where every partial sum is an integer, against ops.hessian_update on each
expert's gathered rows bit for bit (views, graph replay on another routing), through ExpertHessians, and its refusals.  The routings are
made by hand: an empty expert, one row, one full stage, a stage and a row, three stages with a ragged tail; order[] is a random
permutation of the pairs, not ascending inside an expert."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 32, 33, 70)
OTHER = (40, 0, 3, 64, 29)  # a second routing of the same shapes
E, P = len(COUNTS), sum(COUNTS)


def routing(counts, seed, dev):
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    order = torch.from_numpy(np.random.default_rng(seed).permutation(P).astype(np.int32))
    return offsets.to(dev), order.to(dev)


def gathered(x, offsets, order, a_div, e):
    lo, hi = int(offsets[e]), int(offsets[e + 1])
    return x[order[lo:hi].long() // a_div]


@pytest.mark.parametrize("a_div", [1, 2])
@pytest.mark.parametrize("n", [64, 192, 320])
def test_exact_on_small_integers(dev, n, a_div):
    """integers -3 ... 3, powers of two for alpha and beta: every product and partial sum is exact in f32, so every H_e equals
    alpha_e H_e + beta_e X_e^T X_e computed in f64, and its transpose; alpha == 0 drops a NaN-filled matrix, the empty expert keeps its"""
    from qqq_amd.quant import ops

    g = torch.Generator().manual_seed(n + a_div)
    offsets, order = routing(COUNTS, n, dev)
    x = torch.randint(-3, 4, (P // a_div, n), generator=g).half().to(dev)
    up = torch.randint(-3, 4, (E, n, n), generator=g).float().triu()
    H0 = (up + up.triu(1).transpose(1, 2)).to(dev)
    H0[0] = H0[1] = float("nan")
    alpha, beta = [0.5, 0.0, 0.25, 1.0, 2.0], [1.0, 2.0, 0.5, 0.25, 0.125]
    H = ops.hessian_update_grouped(H0.clone(), x, offsets, order, torch.tensor(alpha, device=dev), torch.tensor(beta, device=dev), a_div)
    assert torch.equal(H[0].view(torch.int32), H0[0].view(torch.int32))
    for e in range(1, E):
        xe = gathered(x, offsets, order, a_div, e).double()
        want = beta[e] * (xe.t() @ xe) + (alpha[e] * H0[e].double() if alpha[e] else 0)
        assert torch.equal(H[e].double(), want) and torch.equal(H[e], H[e].t()), e


def test_the_dense_op_s_bits_in_views_and_from_a_replayed_graph(dev):
    from qqq_amd.quant import ops

    n, a_div, g = 192, 2, torch.Generator().manual_seed(5)
    R = P // a_div
    x, x2 = (torch.randn(R, n, generator=g).half().to(dev) for _ in range(2))
    H0 = torch.randn(E, n, n, generator=g).to(dev)
    alpha, beta = [0.3, 0.75, 0.9, 0.5, 0.6], [0.7, 0.4, 0.05, 2.0 / 33, 0.01]
    al, be = torch.tensor(alpha, device=dev), torch.tensor(beta, device=dev)

    def dense(x, offsets, order):
        out = H0.clone()
        for e in range(E):
            rows = gathered(x, offsets, order, a_div, e)
            if rows.shape[0]:
                ops.hessian_update(out[e], rows.contiguous(), alpha[e], beta[e])
        return out

    route1, route2 = routing(COUNTS, 1, dev), routing(OTHER, 2, dev)
    want = dense(x, *route1)
    hbuf = torch.full((E, n + 2, n + 72), 3.0, device=dev)
    xbuf = torch.full((R + 2, n + 24), 5.0, dtype=torch.float16, device=dev)
    hv, xv = hbuf[:, 1:n + 1, 8:n + 8], xbuf[1:R + 1, 8:n + 8]
    hv.copy_(H0)
    xv.copy_(x)
    xkeep = xbuf.clone()
    assert ops.hessian_update_grouped(hv, xv, *route1, al, be, a_div) is hv
    assert torch.equal(hv.view(torch.int32), want.view(torch.int32)) and torch.equal(xbuf, xkeep)
    hv.fill_(3.0)
    assert bool((hbuf == 3.0).all())  # nothing outside the views moved
    # a graph captured on one routing, replayed on another of the same shapes: the eager bits, every time
    hs, xs, offs, ords = H0.clone(), x.clone(), route1[0].clone(), route1[1].clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.hessian_update_grouped(hs, xs, offs, ords, al, be, a_div)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.hessian_update_grouped(hs, xs, offs, ords, al, be, a_div)
    xs.copy_(x2)
    offs.copy_(route2[0])
    ords.copy_(route2[1])
    want2 = dense(x2, *route2)
    assert not torch.equal(want2, want)
    for _ in range(3):
        hs.copy_(H0)
        graph.replay()
        assert torch.equal(hs.view(torch.int32), want2.view(torch.int32))


def test_expert_hessians_over_two_routings(dev):
    """ExpertHessians("fused") is, per expert, the dense op under the Python-float factors n / (n + c) and 2 / (n + c); against the f64
    statement its relative Frobenius error is at most twice that of the f32 steps of "torch" (tests/test_gpu_hessian.py's criterion).
    Measured on an MI355X: error 1.77e-08 against 6.56e-08, ratio 0.27"""
    from qqq_amd.quant import ExpertHessians, ops

    n, g = 192, torch.Generator().manual_seed(9)
    calls = [(torch.randn(P // a, n, generator=g).half(), routing(c, s, "cpu"), a) for c, s, a in ((COUNTS, 3, 2), (OTHER, 4, 1))]
    fused, torch_ = ExpertHessians(E, n, dev, "fused"), ExpertHessians(E, n, "cpu", "torch")
    want, ref, seen = torch.zeros(E, n, n, device=dev), torch.zeros(E, n, n, dtype=torch.float64), [0] * E
    for x, (offsets, order), a_div in calls:
        fused.add_batch(x.to(dev), offsets.to(dev), order.to(dev), a_div)
        torch_.add_batch(x, offsets, order, a_div)
        for e in range(E):
            rows = gathered(x, offsets, order, a_div, e)
            c = rows.shape[0]
            if c:
                ops.hessian_update(want[e], rows.to(dev).contiguous(), seen[e] / (seen[e] + c), 2 / (seen[e] + c))
                ref[e] = ref[e] * (seen[e] / (seen[e] + c)) + (2 / (seen[e] + c)) * (rows.double().t() @ rows.double())
                seen[e] += c
    assert fused.count.tolist() == seen == torch_.count.tolist() == [a + b for a, b in zip(COUNTS, OTHER)]
    assert torch.equal(fused.H.view(torch.int32), want.view(torch.int32))
    rel = lambda H: float((H.double().cpu() - ref).norm() / ref.norm())
    got, bound = rel(fused.H), rel(torch_.H)
    print(f"n {n}: error {got:.3e}, the f32 steps' {bound:.3e}, ratio {got / bound:.3f}")
    assert got <= 2 * bound


def test_every_argument_rejection(dev):
    from qqq_amd.quant import ExpertHessians, _lib, ops

    f = ops.hessian_update_grouped
    n = 128
    H, x = torch.zeros((E, n, n), device=dev), torch.zeros((P, n), dtype=torch.float16, device=dev)
    offsets, order = routing(COUNTS, 0, dev)
    al = be = torch.ones(E, device=dev)
    wide = torch.zeros((E, n, 264), device=dev)
    bad = [
        (lambda: f(H.double(), x, offsets, order, al, be, 1), "hessian_update_grouped: H must be a float32 .E, n, n. tensor"),
        (lambda: f(H[0], x, offsets, order, al, be, 1), "hessian_update_grouped: H must be a float32 .E, n, n. tensor"),
        (lambda: f(H[:, :64], x, offsets, order, al, be, 1), "hessian_update_grouped: H.e. has the shape"),
        (lambda: f(torch.zeros((E, 96, 96), device=dev), x, offsets, order, al, be, 1), "no multiple of 64 in 64 ... 32768"),
        (lambda: f(wide[:, :, 2:130], x, offsets, order, al, be, 1), "hessian_update_grouped: H.e. must be 16-byte aligned"),
        (lambda: f(H.expand(2, E, n, n)[:, 0], x, offsets[:3], order, al[:2], be[:2], 1), "hessian_update_grouped: H must have an expert stride"),
        (lambda: f(H, x.float(), offsets, order, al, be, 1), "hessian_update_grouped: x must be a float16 matrix"),
        (lambda: f(H, x[:, :64], offsets, order, al, be, 1), "hessian_update_grouped: x has the shape"),
        (lambda: f(H, x[:P // 2], offsets, order, al, be, 1), "hessian_update_grouped: x has the shape"),
        (lambda: f(H, x, offsets[:E], order, al, be, 1), "hessian_update_grouped: offsets must be contiguous int32"),
        (lambda: f(H, x, offsets, order.long(), al, be, 1), "hessian_update_grouped: order must be contiguous int32"),
        (lambda: f(H, x, offsets, order, al.double(), be, 1), "hessian_update_grouped: alpha must be contiguous float32"),
        (lambda: f(H, x, offsets, order, al, be[:2], 1), "hessian_update_grouped: beta must be contiguous float32"),
        (lambda: f(H, x, offsets, order, al, be, 0), "hessian_update_grouped: a_div must be an integer >= 1"),
        (lambda: f(H, x, offsets, order.cpu(), al, be, 1), "hessian_update_grouped: every tensor must be on the GPU"),
        (lambda: ExpertHessians(E, n, dev, "lapack"), "ExpertHessians: accumulate must be one of"),
        (lambda: ExpertHessians(E, n, dev, "fused").add_batch(x.float(), offsets, order, 1), "accumulate='fused' takes float16 inputs on the GPU"),
        (lambda: ExpertHessians(E, 64, dev, "fused").add_batch(x, offsets, order, 1), "ExpertHessians.add_batch: the input is"),
    ]
    for call, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            call()
    assert f(H, x, offsets, order[:0], al, be, 1) is H  # P == 0: nothing to do
    # the entry point itself: n, E, P / R, strides, alignment, X inside H
    L, p, q, r = _lib.lib(), H.data_ptr(), x.data_ptr(), (offsets.data_ptr(), order.data_ptr(), al.data_ptr(), be.data_ptr())
    for (lde, ldh, xp, ldx, Pn, R, En, nn, a_div), msg in [
            ((n * n, n, q, n, P, P, E, 96, 1), "qqq_hessian_update_grouped: n=96 is not a multiple of 64"),
            ((n * n, n, q, n, P, P, 0, n, 1), "qqq_hessian_update_grouped: E=0 is not in 1 ... 256"),
            ((n * n, n, q, n, P, P, 257, n, 1), "qqq_hessian_update_grouped: E=257 is not in 1 ... 256"),
            ((n * n, n, q, n, 2097153, 2097153, E, n, 1), "qqq_hessian_update_grouped: bad routing shape"),
            ((n * n, n, q, n, P, P // 2 - 1, E, n, 2), "qqq_hessian_update_grouped: bad routing shape"),
            ((n * n, n, q, n, P, P, E, n, 0), "qqq_hessian_update_grouped: bad routing shape"),
            ((n * n - 4, n, q, n, P, P, E, n, 1), "qqq_hessian_update_grouped: bad strides"),
            ((n * n, 64, q, n, P, P, E, n, 1), "qqq_hessian_update_grouped: bad strides"),
            ((n * n, n, q, 132, P, P, E, n, 1), "qqq_hessian_update_grouped: bad strides"),
            ((n * n, n, q + 8, n, P, P, E, n, 1), "qqq_hessian_update_grouped: bad argument"),
            ((n * n, n, 0, n, P, P, E, n, 1), "qqq_hessian_update_grouped: bad argument"),
            ((n * n, n, p + 256, n, P, P, E, n, 1), "qqq_hessian_update_grouped: H and X overlap")]:
        assert L.qqq_hessian_update_grouped(p, lde, ldh, xp, ldx, *r, Pn, R, En, nn, a_div, 0, None) == _lib.ERR_ARG
        assert _lib.last_error().startswith(msg), _lib.last_error()
    torch.cuda.synchronize()
    assert not H.any() and not wide.any() and not x.any()  # nothing was launched
