"""The q / k norm fused into the RoPE / cache-write ops on the GPU (include_ops/qqq_amd_qknorm.h): all four forms bit for bit against the numpy
restatement (tests/qknorm_ref.py) -- q_out, cached rows, codes and scales, and every slot the call must not touch -- at head layouts that
leave a partial wave (60 items), cross a wave (80 items) and fill whole ones, with q | k | v read in place from one fused buffer, a
position of -1, a position at table_len, a padding slot, all-zero rows and values near the top of fp16.  Then the int8 forms against
quant_rows of what the fp16 forms stored, the v rows against the ops without the norm, and a graph captured once and replayed with new
positions and slots."""
import numpy as np
import pytest
import torch

import qknorm_ref as R

pytestmark = pytest.mark.gpu

LAYOUTS = [(5, 5, 64), (6, 2, 128), (8, 1, 128), (4, 4, 64)]  # (h, kvh, d): 60 items (a partial wave), 80 (crosses a wave), 80, 48
TABLE_LEN, CAP, EPS = 40, 48, 1e-6
SENT, SENT8 = -1234.0, 77  # in every fp16 / f32 and int8 slot the call must not touch


def _bits(t):
    return t.contiguous().view(torch.int16)


def _case(dev, h, kvh, d, m, bs, nb):
    """inputs of one call: views into one fused buffer (row stride (h + 2 kvh) d + 16 > h d), norm weights, tables, positions, slots"""
    g = torch.Generator(device=dev).manual_seed(1000 * h + 10 * kvh + d + m)
    nq, nk = h * d, kvh * d
    amp = torch.exp2(torch.randint(-8, 5, (m, 1), generator=g, device=dev).float())
    buf = torch.zeros((m, nq + 2 * nk + 16), dtype=torch.float16, device=dev)
    buf[:, :nq + 2 * nk] = (torch.randn((m, nq + 2 * nk), generator=g, device=dev) * amp).half()
    buf[0, :d] = 0                                                 # an all-zero q head row
    buf[m - 1, nq:nq + d] = 0                                      # an all-zero k head row
    buf[0, nq + nk:nq + nk + d] = 0                                # an all-zero v head row
    buf[m - 1, (h - 1) * d:nq] = 6.0e4                             # a q head row at the top of fp16 ...
    buf[0, nq + (kvh - 1) * d:nq + nk] = (torch.randn(d, generator=g, device=dev) * 1e-3).half()
    buf[0, nq + (kvh - 1) * d + d // 2 + 3] = -6.2e4               # ... and one such element among small ones in a k head row
    q, k, v = buf[:, :nq], buf[:, nq:nq + nk], buf[:, nq + nk:nq + 2 * nk]
    qw = (1 + 0.3 * torch.randn(d, generator=g, device=dev)).half()
    kw = (1 + 0.3 * torch.randn(d, generator=g, device=dev)).half()
    cos = (torch.rand((TABLE_LEN, d), generator=g, device=dev) * 2 - 1).half()
    sin = (torch.rand((TABLE_LEN, d), generator=g, device=dev) * 2 - 1).half()
    if m == 1:
        pos, slots = [3], [bs + 3]
    else:  # token 1 at position -1, token 3 at table_len (both write nothing), token 5 with a padding slot (q_out only)
        pos = [3, -1, 17, TABLE_LEN, 0, 9, TABLE_LEN - 1]
        slots = [5, 20, bs + 3, 2 * bs - 2, 0, -1, bs * nb - 1]
    pos, slots = torch.tensor(pos, device=dev), torch.tensor(slots, device=dev)
    return q, k, v, qw, kw, cos, sin, pos, slots


def _reference(q, k, v, qw, kw, cos, sin, pos, h, kvh, d):
    """(q_rows [m, h, d], k_rows, v_rows [m, kvh, d] fp16 numpy, valid [m] bool): the restatement, computed once per case"""
    p = pos.cpu().numpy()
    valid = (p >= 0) & (p < TABLE_LEN)
    qr, kr, vr = R.rope_qkv_norm(q.cpu().numpy(), k.cpu().numpy(), v.cpu().numpy(), qw.cpu().numpy(), kw.cpu().numpy(), EPS,
                                 cos.cpu().numpy(), sin.cpu().numpy(), np.where(valid, p, 0), h, kvh, d)
    return qr, kr, vr, valid


def _eq16(got, want):
    return np.array_equal(got.cpu().numpy().view(np.uint16), np.ascontiguousarray(want).view(np.uint16))


@pytest.mark.parametrize("m", [1, 7])
@pytest.mark.parametrize("h,kvh,d", LAYOUTS)
def test_all_four_forms_are_the_restatement_bit_for_bit(dev, h, kvh, d, m):
    from qqq_amd import ops

    for bs, nb in ((16, 6), (256, 2)):
        q, k, v, qw, kw, cos, sin, pos, slots = _case(dev, h, kvh, d, m, bs, nb)
        assert q.stride(0) > h * d and k.data_ptr() == q.data_ptr() + 2 * h * d  # views into the one buffer, read in place
        qr, kr, vr, valid = _reference(q, k, v, qw, kw, cos, sin, pos, h, kvh, d)
        p, sl = pos.cpu().numpy(), slots.cpu().numpy()
        what = (h, kvh, d, m, bs)
        assert (kr[valid] != 0).any() and np.isfinite(qr[valid].astype(np.float32)).all()

        # ---- the block pools
        cached = valid & (sl >= 0) & (sl < nb * bs)
        want_k = np.full((nb, kvh, bs, d), SENT, np.float16)
        want_v = want_k.copy()
        want_k8, want_ks = np.full((nb, kvh, bs, d), SENT8, np.int8), np.full((nb, kvh, bs), SENT, np.float32)
        want_v8, want_vs = want_k8.copy(), want_ks.copy()
        for t in np.nonzero(cached)[0]:
            blk, off = sl[t] // bs, sl[t] % bs
            want_k[blk, :, off], want_v[blk, :, off] = kr[t], vr[t]
            want_k8[blk, :, off], want_ks[blk, :, off] = R.quant(kr[t])
            want_v8[blk, :, off], want_vs[blk, :, off] = R.quant(vr[t])
        kp = torch.full((nb, kvh, bs, d), SENT, dtype=torch.float16, device=dev)
        vp = kp.clone()
        q_out = ops.rope_qkv_norm_paged(q, k, v, qw, kw, EPS, cos, sin, pos, slots, kp, vp)
        assert q_out.shape == (m, h, d) and q_out.is_contiguous()
        assert _eq16(q_out[torch.from_numpy(valid).to(dev)], qr[valid]), what
        assert _eq16(kp, want_k) and _eq16(vp, want_v), what
        kp8 = torch.full((nb, kvh, bs, d), SENT8, dtype=torch.int8, device=dev)
        ksp = torch.full((nb, kvh, bs), SENT, dtype=torch.float32, device=dev)
        vp8, vsp = kp8.clone(), ksp.clone()
        q_out8 = ops.rope_qkv_norm_paged_kv8(q, k, v, qw, kw, EPS, cos, sin, pos, slots, kp8, vp8, ksp, vsp)
        assert _eq16(q_out8[torch.from_numpy(valid).to(dev)], qr[valid]), what
        assert np.array_equal(kp8.cpu().numpy(), want_k8) and np.array_equal(vp8.cpu().numpy(), want_v8), what
        assert np.array_equal(ksp.cpu().numpy().view(np.uint32), want_ks.view(np.uint32)), what
        assert np.array_equal(vsp.cpu().numpy().view(np.uint32), want_vs.view(np.uint32)), what
        # the int8 form stores exactly quant_rows of the row the fp16 form stores
        rows = torch.from_numpy(np.nonzero(cached)[0])
        for pool16, pool8, scale in ((kp, kp8, ksp), (vp, vp8, vsp)):
            for t in rows.tolist():
                blk, off = sl[t] // bs, sl[t] % bs
                codes, scales = R.quant(pool16[blk, :, off].cpu().numpy())
                assert np.array_equal(pool8[blk, :, off].cpu().numpy(), codes), what
                assert np.array_equal(scale[blk, :, off].cpu().numpy().view(np.uint32), scales.view(np.uint32)), what
        # v is untouched by the norm: the pools' v rows are rope_qkv_paged's and rope_qkv_paged_kv8's
        kp0 = torch.full((nb, kvh, bs, d), SENT, dtype=torch.float16, device=dev)
        vp0 = kp0.clone()
        ops.rope_qkv_paged(q, k, v, cos, sin, pos, slots, kp0, vp0)
        assert torch.equal(_bits(vp0), _bits(vp)), what
        assert not torch.equal(_bits(kp0), _bits(kp)), what  # and the norm is no no-op on k
        kq0 = torch.full((nb, kvh, bs, d), SENT8, dtype=torch.int8, device=dev)
        ks0 = torch.full((nb, kvh, bs), SENT, dtype=torch.float32, device=dev)
        vq0, vs0 = kq0.clone(), ks0.clone()
        ops.rope_qkv_paged_kv8(q, k, v, cos, sin, pos, slots, kq0, vq0, ks0, vs0)
        assert torch.equal(vq0, vp8) and torch.equal(vs0.view(torch.int32), vsp.view(torch.int32)), what

        if bs != 16:
            continue
        # ---- the static caches: one row of m tokens, and m rows of one token
        for b, s in ((1, m), (m, 1)):
            want_k = np.full((b, kvh, CAP, d), SENT, np.float16)
            want_v = want_k.copy()
            want_k8, want_ks = np.full((b, kvh, CAP, d), SENT8, np.int8), np.full((b, kvh, CAP), SENT, np.float32)
            want_v8, want_vs = want_k8.copy(), want_ks.copy()
            want_q = np.zeros((b, h, s, d), np.float16)
            mask = np.zeros((b, h, s, d), bool)
            for t in np.nonzero(valid)[0]:
                bi, si = t // s, t % s
                want_q[bi, :, si], mask[bi, :, si] = qr[t], True
                want_k[bi, :, p[t]], want_v[bi, :, p[t]] = kr[t], vr[t]
                want_k8[bi, :, p[t]], want_ks[bi, :, p[t]] = R.quant(kr[t])
                want_v8[bi, :, p[t]], want_vs[bi, :, p[t]] = R.quant(vr[t])
            kc = torch.full((b, kvh, CAP, d), SENT, dtype=torch.float16, device=dev)
            vc = kc.clone()
            q_out = ops.rope_qkv_norm(q, k, v, qw, kw, EPS, cos, sin, pos, kc, vc)
            assert q_out.shape == (b, h, s, d)
            assert np.array_equal(q_out.cpu().numpy().view(np.uint16)[mask], want_q.view(np.uint16)[mask]), (what, b, s)
            assert _eq16(kc, want_k) and _eq16(vc, want_v), (what, b, s)
            kc8 = torch.full((b, kvh, CAP, d), SENT8, dtype=torch.int8, device=dev)
            ksc = torch.full((b, kvh, CAP), SENT, dtype=torch.float32, device=dev)
            vc8, vsc = kc8.clone(), ksc.clone()
            q_out8 = ops.rope_qkv_norm_kv8(q, k, v, qw, kw, EPS, cos, sin, pos, kc8, vc8, ksc, vsc)
            assert np.array_equal(q_out8.cpu().numpy().view(np.uint16)[mask], want_q.view(np.uint16)[mask]), (what, b, s)
            assert np.array_equal(kc8.cpu().numpy(), want_k8) and np.array_equal(vc8.cpu().numpy(), want_v8), (what, b, s)
            assert np.array_equal(ksc.cpu().numpy().view(np.uint32), want_ks.view(np.uint32)), (what, b, s)
            assert np.array_equal(vsc.cpu().numpy().view(np.uint32), want_vs.view(np.uint32)), (what, b, s)
            vc0 = torch.full((b, kvh, CAP, d), SENT, dtype=torch.float16, device=dev)
            ops.rope_qkv(q, k, v, cos, sin, pos, vc0.clone(), vc0)
            assert torch.equal(_bits(vc0), _bits(vc)), (what, b, s)


def test_no_tokens_is_a_no_op_and_bad_arguments_are_refused_before_any_launch(dev):
    from qqq_amd import ops

    h, kvh, d, bs, nb = 6, 2, 128, 16, 2
    q, k, v, qw, kw, cos, sin, pos, slots = _case(dev, h, kvh, d, 1, bs, nb)
    kp = torch.full((nb, kvh, bs, d), SENT, dtype=torch.float16, device=dev)
    vp = kp.clone()
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    out = ops.rope_qkv_norm_paged(q[:0], k[:0], v[:0], qw, kw, EPS, cos, sin, none, none, kp, vp)
    assert out.shape[0] == 0 and bool((kp == SENT).all()) and bool((vp == SENT).all())
    with pytest.raises(RuntimeError, match=r"q_weight .* must be fp16 \[128\]"):
        ops.rope_qkv_norm_paged(q, k, v, qw[:64], kw, EPS, cos, sin, pos, slots, kp, vp)
    with pytest.raises(RuntimeError, match="eps"):
        ops.rope_qkv_norm_paged(q, k, v, qw, kw, -1.0, cos, sin, pos, slots, kp, vp)
    with pytest.raises(RuntimeError, match="norm weights must be fp16"):
        ops.rope_qkv_norm_paged(q, k, v, qw.float(), kw, EPS, cos, sin, pos, slots, kp, vp)
    d32 = 32
    with pytest.raises(RuntimeError, match="head_dim 32"):
        kc = torch.zeros((1, 1, 8, d32), dtype=torch.float16, device=dev)
        z = torch.zeros((1, d32), dtype=torch.float16, device=dev)
        ops.rope_qkv_norm(z, z, z, torch.ones(d32, dtype=torch.float16, device=dev), torch.ones(d32, dtype=torch.float16, device=dev), EPS,
                          torch.zeros((8, d32), dtype=torch.float16, device=dev), torch.zeros((8, d32), dtype=torch.float16, device=dev),
                          torch.zeros(1, dtype=torch.int64, device=dev), kc, kc.clone())
    assert bool((kp == SENT).all()) and bool((vp == SENT).all())


@pytest.mark.parametrize("kv8", [False, True])
def test_a_graph_captured_once_replays_with_new_positions_and_slots(dev, kv8):
    from qqq_amd import ops

    h, kvh, d, bs, nb, m = 6, 2, 128, 16, 6, 7
    q, k, v, qw, kw, cos, sin, pos0, slots0 = _case(dev, h, kvh, d, m, bs, nb)

    def pools():
        if kv8:
            return (torch.full((nb, kvh, bs, d), SENT8, dtype=torch.int8, device=dev), torch.full((nb, kvh, bs, d), SENT8, dtype=torch.int8, device=dev),
                    torch.full((nb, kvh, bs), SENT, dtype=torch.float32, device=dev), torch.full((nb, kvh, bs), SENT, dtype=torch.float32, device=dev))
        return (torch.full((nb, kvh, bs, d), SENT, dtype=torch.float16, device=dev), torch.full((nb, kvh, bs, d), SENT, dtype=torch.float16, device=dev))

    op = ops.rope_qkv_norm_paged_kv8 if kv8 else ops.rope_qkv_norm_paged
    pg, pe = pools(), pools()
    pos = torch.zeros(m, dtype=torch.int64, device=dev)
    slots = torch.full((m,), -1, dtype=torch.int64, device=dev)  # the warm-up and the capture write no cache row
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op(q, k, v, qw, kw, EPS, cos, sin, pos, slots, *pg)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = op(q, k, v, qw, kw, EPS, cos, sin, pos, slots, *pg)
    torch.cuda.current_stream().wait_stream(side)
    for new_pos, new_slots in ((pos0, slots0), (torch.tensor([7, 8, 9, 10, -1, 12, 39], device=dev), torch.tensor([40, 41, 42, -1, 44, 45, 46], device=dev))):
        pos.copy_(new_pos)
        slots.copy_(new_slots)
        graph.replay()
        torch.cuda.synchronize()
        want = op(q, k, v, qw, kw, EPS, cos, sin, pos, slots, *pe)
        ok = ((pos >= 0) & (pos < TABLE_LEN))
        assert torch.equal(_bits(out[ok]), _bits(want[ok])), kv8
        for a, b_ in zip(pg, pe):
            assert torch.equal(a.contiguous().view(torch.int8), b_.contiguous().view(torch.int8)), kv8
        assert bool((pg[0] != (SENT8 if kv8 else SENT)).any())  # the replay wrote rows
