"""Decoder-block activation quantisers (rmsnorm_quant, silu_mul_quant), QuantLinear.forward_int8 and the block modules on the GPU."""
import pytest
import torch
import torch.nn.functional as F

import act_ref as R

pytestmark = pytest.mark.gpu

MS = (1, 7, 16, 300, 4099)
KS = (8, 4096, 5120, 8192, 11008, 13824, 28672, 65536)
EPS = 1e-6


def _rows_with_specials(m, k, g, dev, scale=1.0):
    """randn rows; row 0 all zero, row 1 near +-fp16 max, row 2 one outlier (where the rows exist)"""
    x = (torch.randn((m, k), generator=g, device=dev) * scale).half()
    if m > 0:
        x[0] = 0
    if m > 1:
        x[1] = ((torch.rand(k, generator=g, device=dev) * 2 - 1) * 65000).half()
    if m > 2:
        x[2, k // 3] = 3000 * scale
    return x


def _check_quant_contract(xq, s1, y, what):
    from qqq_amd import ops

    dq, ds = ops.dynamic_quant(y)
    assert torch.equal(ds.view(torch.int32), s1.view(torch.int32)), what
    assert torch.equal(dq, xq), what


def _ulp_report(name, d, extra=0):
    n = d.numel()
    frac = float((d != 0).sum().item()) / n
    print(f"{name}: y not bit-equal to torch at {frac:.3e} of {n} elements (max {int(d.max().item())} ulp; {extra} of them two-rounding 2 ulp)")


@pytest.mark.parametrize("k", KS)
def test_rmsnorm_quant(dev, k):
    from qqq_amd import ops

    g = torch.Generator(device=dev).manual_seed(k)
    w = (1 + 0.1 * torch.randn(k, generator=g, device=dev)).half()
    for m in MS:
        x = _rows_with_specials(m, k, g, dev)
        for with_res in (False, True):
            r0 = None
            if with_res:
                r0 = (torch.randn((m, k), generator=g, device=dev) * 2).half()
                r0[: min(m, 2)] = 0  # the zero and near-max rows stay what they are (no fp16 overflow in the add)
            r = None if r0 is None else r0.clone()
            xq, s1, y = ops.rmsnorm_quant(x, w, EPS, residual=r, return_y=True)
            _check_quant_contract(xq, s1, y, (m, k, with_res))
            if with_res:
                assert torch.equal(r.view(torch.int16), (r0 + x).view(torch.int16)), (m, k)  # torch's fp16 `+`, bit for bit
            # the same call without storing y: the same codes / scales
            r2 = None if r0 is None else r0.clone()
            xq2, s12 = ops.rmsnorm_quant(x, w, EPS, residual=r2)
            assert torch.equal(xq2, xq) and torch.equal(s12, s1)
            if with_res:
                assert torch.equal(r2, r)
            # against torch: y is torch's expression applied to an n within one fp16 ulp of torch's n.  The fp32 sum of squares is reduced
            # in another order than torch's, so rsqrt(var + eps) may differ in its last bit; where that moves n = fp16(h * rsqrt) to the
            # neighbouring fp16 value, the second rounding y = fp16(w * n) can land 2 ulps from torch's y.  Everywhere else: <= 1 ulp.
            ty, tn, _ = R.torch_rmsnorm(x, w, EPS, residual=r0)
            d = R.ulp_diff(y, ty)
            far = d > 1
            n_far = int(far.sum().item())
            if n_far:
                o = R.ordered(tn)
                wf = w.expand_as(tn)
                cand = [(wf * R.from_ordered(o + s)).view(torch.int16) for s in (-1, 1)]
                ok = (y.view(torch.int16) == cand[0]) | (y.view(torch.int16) == cand[1])
                assert bool(ok[far].all()), (m, k, with_res, int(d.max().item()))
            _ulp_report(f"rmsnorm_quant m={m} k={k} residual={with_res}", d, n_far)
            assert n_far <= max(1, d.numel() // 1000), (m, k, n_far)
            del xq, s1, y, ty, tn, d, xq2, s12


@pytest.mark.parametrize("i", KS)
def test_silu_mul_quant(dev, i):
    from qqq_amd import ops

    g = torch.Generator(device=dev).manual_seed(1000 + i)
    for m in MS:
        gu = torch.empty((m, 2 * i), dtype=torch.float16, device=dev)
        gu[:, :i] = _rows_with_specials(m, i, g, dev, scale=3.0)
        gu[:, i:] = (torch.randn((m, i), generator=g, device=dev)).clamp(-1, 1).half()  # |up| <= 1: the near-max gate row stays finite
        gate, up = gu[:, :i], gu[:, i:]
        xq, s1, y = ops.silu_mul_quant(gate, up, return_y=True)  # strided halves of one fused output, read in place
        _check_quant_contract(xq, s1, y, (m, i))
        gs, us = gate.contiguous(), up.contiguous()  # two separate tensors
        xq2, s12, y2 = ops.silu_mul_quant(gs, us, return_y=True)
        assert torch.equal(y2.view(torch.int16), y.view(torch.int16)) and torch.equal(xq2, xq) and torch.equal(s12, s1)
        xq3, s13 = ops.silu_mul_quant(gate, up)
        assert torch.equal(xq3, xq) and torch.equal(s13, s1)
        d = R.ulp_diff(y, R.torch_silu_mul(gate, up))
        _ulp_report(f"silu_mul_quant m={m} i={i}", d)
        assert int(d.max().item()) <= 1, (m, i)
        del gu, xq, s1, y, y2, xq2, gs, us, d


def _make_ql(dev, K, N, group_size, bias, seed):
    from qqq_amd import QuantLinear, pack as P

    g = torch.Generator(device=dev).manual_seed(seed)
    ql = QuantLinear(4, group_size, K, N, bias=bias).to(dev)
    if group_size != -1:
        codes = torch.randint(0, 16, (K, N), generator=g, dtype=torch.int8, device=dev)
        ql.s_group.copy_((torch.rand((K // 128, N), generator=g, device=dev) * 1.5 + 0.05).half())
    else:
        codes = torch.randint(-7, 8, (K, N), generator=g, dtype=torch.int8, device=dev)
    ql.B.copy_(P.pack_codes(codes, group_size != -1))
    ql.s_channel.copy_(torch.rand((1, N), generator=g, device=dev) * 2e-4 + 1e-5)
    if bias:
        ql.bias.copy_((torch.randn(N, generator=g, device=dev) * 0.1).half())
    return ql


@pytest.mark.parametrize("group_size", [-1, 128])
def test_forward_int8_equals_forward(dev, group_size):
    from qqq_amd import ops

    K, N = 4096, 4096
    for bias in (False, True):
        ql = _make_ql(dev, K, N, group_size, bias, seed=7 + bias)
        for w8 in (False, True):
            if w8:
                ql.expand_for_prefill(per_channel=True)
            for m in (1, 16, 128, 1024):
                x = (torch.randn((m, K), device=dev) * 1.3).half()
                a = ql.forward(x)
                b = ql.forward_int8(*ops.dynamic_quant(x))
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (group_size, bias, w8, m)
            x3 = (torch.randn((2, 3, K), device=dev)).half()
            b3 = ql.forward_int8(*ops.dynamic_quant(x3))
            assert b3.shape == (2, 3, N) and torch.equal(b3.view(torch.int16), ql.forward(x3).view(torch.int16))
        ql.drop_expanded()


def _make_mlp(dev, hidden, inter, group_size, seed):
    from qqq_amd import QuantLlamaMLP

    mlp = QuantLlamaMLP(hidden, inter, group_size).to(dev)
    mlp.gate_proj = _make_ql(dev, hidden, inter, group_size, False, seed)
    mlp.up_proj = _make_ql(dev, hidden, inter, group_size, False, seed + 1)
    mlp.down_proj = _make_ql(dev, inter, hidden, group_size, False, seed + 2)
    return mlp


@pytest.mark.parametrize("group_size", [-1, 128])
def test_mlp(dev, group_size):
    from qqq_amd import ops

    hidden, inter = 4096, 11008
    mlp = _make_mlp(dev, hidden, inter, group_size, seed=20)
    for m in (1, 16, 128, 1024):
        x = torch.randn((m, hidden), device=dev).half()
        xq, s1 = ops.dynamic_quant(x)
        # the composition of existing pieces
        gt, ut = mlp.gate_proj.forward_int8(xq, s1), mlp.up_proj.forward_int8(xq, s1)
        _, _, y = ops.silu_mul_quant(gt, ut, return_y=True)
        want = mlp.down_proj.forward_int8(*ops.dynamic_quant(y))
        mlp.unfuse_gate_up()
        got = mlp.forward_int8(xq, s1)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (group_size, m)
        mlp.fuse_gate_up()
        got_f = mlp.forward_int8(xq, s1)
        assert torch.equal(got_f.view(torch.int16), want.view(torch.int16)), (group_size, m, "fused")
        assert torch.equal(mlp.forward(x).view(torch.int16), want.view(torch.int16))
        # against the pure-torch expression built from QuantLinear.forward: only silu * up may differ (<= 1 ulp), then re-quantised
        ref = mlp.down_proj.forward(F.silu(mlp.gate_proj.forward(x)) * mlp.up_proj.forward(x))
        rel = float((got.float() - ref.float()).norm() / ref.float().norm())
        print(f"QuantLlamaMLP g={group_size} m={m}: relative L2 error vs torch silu*up composition {rel:.2e}")
        assert torch.isfinite(got).all() and rel <= 1e-2, rel


def test_fuse_gate_up_memory_and_state_dict(dev):
    import gc

    mlp = _make_mlp(dev, 1024, 2816, 128, seed=40)
    sd0 = {k: v.clone() for k, v in mlp.state_dict().items()}
    gu_bytes = sum(t.numel() * t.element_size() for l in (mlp.gate_proj, mlp.up_proj) for t in (l.B, l.s_channel, l.s_group))
    gc.collect()  # earlier tests' garbage must not be freed inside the measured region
    gc.disable()
    try:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        mlp.fuse_gate_up()
        grown = torch.cuda.memory_allocated(dev) - before
        assert grown >= gu_bytes  # a second copy of gate/up (+ the fused layer's own scratch buffers)
        mlp.unfuse_gate_up()
        assert torch.cuda.memory_allocated(dev) == before  # released at once, no garbage collection needed
        mlp.fuse_gate_up()
        sd = mlp.state_dict()
        assert set(sd) == set(sd0) and all(torch.equal(sd[k], sd0[k]) for k in sd)
        mlp.load_state_dict(sd0)
        assert not mlp.gate_up_fused
        assert torch.cuda.memory_allocated(dev) == before
        del mlp, sd  # the module holds no reference cycle: its device memory goes with the last reference
        sd0.clear()
        assert torch.cuda.memory_allocated(dev) < before - gu_bytes
    finally:
        gc.enable()


def test_rmsnorm_module_residual(dev):
    from qqq_amd import QuantRMSNorm, ops

    k = 4096
    norm = QuantRMSNorm(k, eps=1e-5).to(dev)
    norm.weight.data = (1 + 0.1 * torch.randn(k, device=dev)).half()
    x = torch.randn((5, k), device=dev).half()
    r = torch.randn((5, k), device=dev).half()
    r_in = r.clone()
    xq, s1 = norm(x, r)
    assert torch.equal(r, r_in + x)
    wq, ws, _ = ops.rmsnorm_quant(x, norm.weight, 1e-5, residual=r_in.clone(), return_y=True)
    assert torch.equal(xq, wq) and torch.equal(s1, ws)


def test_ops_trace_under_torch_compile(dev):
    from qqq_amd import ops

    def f(x, w, r, gu):
        xq, s1 = ops.rmsnorm_quant(x, w, EPS, residual=r)
        i = gu.shape[-1] // 2
        hq, hs = ops.silu_mul_quant(gu[:, :i], gu[:, i:])
        return xq, s1, hq, hs

    x = torch.randn((16, 4096), device=dev).half()
    w = (1 + 0.1 * torch.randn(4096, device=dev)).half()
    r = torch.randn((16, 4096), device=dev).half()
    gu = torch.randn((16, 2 * 11008), device=dev).half()
    r_e, r_c = r.clone(), r.clone()
    eager = f(x, w, r_e, gu)
    comp = torch.compile(f, fullgraph=True)(x, w, r_c, gu)
    for a, b in zip(eager, comp):
        assert torch.equal(a, b)
    assert torch.equal(r_e, r_c) and torch.equal(r_e, r + x)


def test_mlp_traces_under_torch_compile(dev):
    mlp = _make_mlp(dev, 1024, 2816, -1, seed=50).fuse_gate_up()
    x = torch.randn((16, 1024), device=dev).half()
    eager = mlp(x)
    comp = torch.compile(mlp, fullgraph=True)(x)
    assert torch.equal(eager.view(torch.int16), comp.view(torch.int16))


def test_mlp_hipgraph_capture_and_replay(dev):
    from qqq_amd import QuantRMSNorm

    hidden, inter = 4096, 11008
    mlp = _make_mlp(dev, hidden, inter, 128, seed=60).fuse_gate_up()
    norm = QuantRMSNorm(hidden).to(dev)
    x = torch.randn((1, hidden), device=dev).half()
    res = torch.randn((1, hidden), device=dev).half()
    r_eager = res.clone()
    want = mlp.forward_int8(*norm(x, r_eager))
    r_graph = res.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mlp.forward_int8(*norm(x, r_graph.clone()))  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = mlp.forward_int8(*norm(x, r_graph))
    torch.cuda.current_stream().wait_stream(side)
    r_graph.copy_(res)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert torch.equal(r_graph, r_eager)
