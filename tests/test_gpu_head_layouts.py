"""The attention kernels at every head layout the headers promise (include/qqq_amd_decode.h, qqq_amd_paged.h, qqq_amd_prefill.h:
h / kvh <= 8, d 64 or 128, h*d <= 16384), beyond the h*d <= 4096 and G = h / kvh in {1, 4, 7} of the other files: all G from 1 to 8
(the prefill tile of 128 / G tokens leaves idle rows at G = 3, 5, 6; the decode split kernel pads Q^T from G to 16 rows), and h*d on
both sides of 4096 and 8192, where the quantising kernels (qqq_decode_combine_kernel, qqq_prefill_quant_kernel) change from one to two
to four 16-byte vectors per thread.

The bounds are those of tests/test_gpu_decode_attn.py and tests/test_gpu_kv8.py for this arithmetic: relative L2 per (row, head) <= 1e-3
and max error <= 2^-9 max|v| over the keys attended, against float64 attention (over the dequantised cache for int8).  The per-head
arithmetic does not depend on h, so no layout has a looser one.  (xq, s1) of a call are held to quant_ref.quant_rows_exact of the o_fp16
it returned, and to dynamic_quant of it."""
import numpy as np
import pytest
import torch

import kv8_ref as K8
import quant_ref as Q
import test_gpu_decode_attn as DEC
import test_gpu_kv8 as KV8
import test_gpu_prefill as PF
from test_gpu_paged import _assert_same, _both, _i32, _poisoned, _shuffled_table, _to_pool

pytestmark = pytest.mark.gpu

#          h, kvh, d        G   h*d    vectors per thread of the quantising kernels
LAYOUTS = [(24, 8, 128),    # 3   3072  1   Llama-3.2-3B
           (33, 11, 128),   # 3   4224  2   one head past 4096
           (40, 8, 128),    # 5   5120  2   Qwen2.5-14B
           (40, 40, 128),   # 1   5120  2   Llama-2-13B
           (64, 8, 128),    # 8   8192  2   the upper end of two; Llama-3-70B
           (65, 13, 128),   # 5   8320  4   one head past 8192
           (96, 16, 128),   # 6  12288  4
           (128, 16, 128),  # 8  16384  4   the maximum
           (16, 8, 64),     # 2   1024  1
           (96, 16, 64),    # 6   6144  2
           (128, 64, 64)]   # 2   8192  2
ONE_PER_G = [(16, 8, 64), (24, 8, 128), (40, 8, 128), (96, 16, 64), (64, 8, 128)]  # G = 2, 3, 5, 6, 8
ERR_ARG = 17  # QQQ_ERR_ARG, include/qqq_amd.h


def _assert_quant_exact(xq, s1, o, what):
    """(xq, s1) against the exact quantiser and against dynamic_quant of the fp16 rows o"""
    from qqq_amd import ops

    q, s = Q.quant_rows_exact(o.cpu().numpy())
    assert np.array_equal(s1.cpu().numpy().view(np.uint32), s.view(np.uint32)), (what, "scales")
    assert np.array_equal(xq.cpu().numpy(), q), (what, "codes", int((xq.cpu().numpy() != q).sum()))
    wq, ws = ops.dynamic_quant(o.contiguous())
    assert torch.equal(xq, wq) and torch.equal(_i32(s1), _i32(ws)), what


def _decode_caches(dev, g, b, kvh, d, cap, kv8):
    k = torch.randn((b, kvh, cap, d), generator=g, device=dev).half()
    v = torch.randn((b, kvh, cap, d), generator=g, device=dev).half()
    if not kv8:
        return (k, v)
    kc, ks = K8.quant_rows_op(k)
    vc, vs = K8.quant_rows_op(v)
    return (kc, vc, ks, vs)


def _decode_pools(g, cont, bs, kv8):
    """the pool that holds the rows of `cont` through a shuffled table, and the id of a poison block no row owns"""
    b, _, cap = cont[0].shape[:3]
    table, nb, spare = _shuffled_table(g, b, cap // bs, cont[0].device, spare=1)
    fills = (127, 127, float("nan"), float("nan")) if kv8 else (float("nan"), float("nan"))
    return tuple(_to_pool(t, table, nb, f) for t, f in zip(cont, fills)), table, int(spare[0])


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("h,kvh,d", LAYOUTS)
def test_decode_attention_against_float64_and_paged_bit_exact(dev, h, kvh, d, kv8):
    from qqq_amd import ops

    b, cap = 3, 1152  # nine 128-key chunks
    g = torch.Generator(device=dev).manual_seed(h * 7 + kvh + d)
    cont = _decode_caches(dev, g, b, kvh, d, cap, kv8)
    q = torch.randn((b, h, 1, d), generator=g, device=dev).half()
    c = DEC._chunk(dev, b, kvh, cap)
    assert -(-cap // c) >= 3, c  # at least three splits
    scale = d ** -0.5
    if kv8:
        k64, v64 = K8.dequant64(cont[0], cont[2]), K8.dequant64(cont[1], cont[3])
    else:
        k64, v64 = cont[0].double(), cont[1].double()
    paged = [(bs,) + _decode_pools(g, cont, bs, kv8) for bs in (16, 128)]
    for p in [(0, 1, c - 1), (c, c + 1, cap - 1), (cap - 1, 17, 2 * c + 5)]:
        pos = torch.tensor(p, dtype=torch.int64, device=dev)
        what = f"decode_attention{'_kv8' if kv8 else ''} h={h} kvh={kvh} d={d} chunk={c} pos={p}"
        if kv8:
            xq, s1, o = ops.decode_attention_kv8(q, *cont, pos, scale, return_fp16=True)
        else:
            xq, s1, o = ops.decode_attention(q, *cont, pos, scale, return_fp16=True)
        torch.cuda.synchronize()
        assert torch.isfinite(o).all(), what
        ref = K8.attention64(q, k64, v64, pos, scale)
        rel, mx = KV8._errors(o, ref, v64, pos)
        srel, smx = KV8._errors(DEC._sdpa(q, k64.half(), v64.half(), pos, scale), ref, v64, pos)
        print(f"{what}: rel L2 {rel:.2e}, max|err|/max|v| {mx:.2e} (2^-9 = {2 ** -9:.2e});  SDPA {srel:.2e}, {smx:.2e}")
        assert rel <= 1e-3 and mx <= 2 ** -9, (what, rel, mx)
        _assert_quant_exact(xq, s1, o, what)
        for bs, pools, table, poison in paged:
            got, want = _both(q, cont, pools, _poisoned(table, pos, bs, poison), pos, scale, cap, kv8)
            _assert_same(want, (xq, s1, o), (what, "the contiguous op twice"))
            _assert_same(got, want, (what, f"paged, block_size {bs}"))


STEP = [(0, 1), (0, 133), (13, 65), (250, 64), (300, 1)]  # 133 is more than two tiles at every G (a tile is at most 64 tokens), 65 straddles one
PAD = 3


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("h,kvh,d", LAYOUTS)
def test_prefill_packed_step_against_float64(dev, h, kvh, d, kv8):
    bs = 16
    g = torch.Generator(device=dev).manual_seed(h * 5 + kvh + d)
    lens = [s + c for s, c in STEP]
    cont = PF._cont(dev, g, lens, kvh, d, 320, kv8)
    pools, table = PF._pools(g, cont, lens, bs, kv8)
    m = sum(c for _, c in STEP)
    q = torch.randn((m + PAD, h, d), generator=g, device=dev).half()
    cu, sp = PF._meta(dev, STEP)
    xq, s1, o = PF._run(q, pools, table, cu, sp, d ** -0.5, kv8)
    assert xq.shape == (m + PAD, h * d) and s1.shape == (m + PAD, 1) and o.shape == (m + PAD, h * d)
    assert torch.isfinite(o[:m].float()).all() and torch.isfinite(s1[:m]).all()
    k64, v64 = PF._kv64(cont, kv8)
    ref, vmax = PF._ref64(q, k64, v64, STEP, d ** -0.5)
    rel, mx = PF._errors(o[:m], ref, vmax)
    srel, smx = PF._errors(PF._sdpa(q, k64.half(), v64.half(), STEP, d ** -0.5), ref, vmax)
    what = f"prefill_attention_paged{'_kv8' if kv8 else ''} h={h} kvh={kvh} d={d}"
    print(f"{what}: rel L2 {rel:.2e}, max|err|/max|v| {mx:.2e} (2^-9 = {2 ** -9:.2e});  SDPA over the gathered copy {srel:.2e}, {smx:.2e}")
    assert rel <= 1e-3 and mx <= 2 ** -9, (what, rel, mx)
    _assert_quant_exact(xq[:m], s1[:m], o[:m], what)


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("h,kvh,d", ONE_PER_G)
def test_prefill_bit_exact_invariances(dev, h, kvh, d, kv8):
    """o_fp16, xq and s1 of a token do not depend on the rest of the batch, on how its sequence is cut into steps, or on the block size"""
    g = torch.Generator(device=dev).manual_seed(h + kvh + d)
    seqs = [(40, 9), (0, 133), (77, 50)]
    lens = [s + c for s, c in seqs]
    cont = PF._cont(dev, g, lens, kvh, d, 256, kv8)
    m = sum(c for _, c in seqs)
    q = torch.randn((m, h, d), generator=g, device=dev).half()
    cu, sp = PF._meta(dev, seqs)
    scale = d ** -0.5
    pools, table = PF._pools(g, cont, lens, 16, kv8)
    base = PF._run(q, pools, table, cu, sp, scale, kv8)
    assert torch.isfinite(base[2].float()).all()
    _assert_quant_exact(*base, (h, kvh, d, kv8))
    pools128, table128 = PF._pools(g, cont, lens, 128, kv8)
    PF._same(PF._run(q, pools128, table128, cu, sp, scale, kv8), base, slice(None), slice(None), "block_size 128")
    alone = PF._run(q[9:142].contiguous(), pools, table[1:2], *PF._meta(dev, seqs[1:2]), scale, kv8)
    PF._same(alone, base, slice(None), slice(9, 142), "alone")
    first = PF._run(q[9:79].contiguous(), pools, table[1:2], *PF._meta(dev, [(0, 70)]), scale, kv8)
    second = PF._run(q[79:142].contiguous(), pools, table[1:2], *PF._meta(dev, [(70, 63)]), scale, kv8)
    PF._same(first, base, slice(None), slice(9, 79), "step of 70")
    PF._same(second, base, slice(None), slice(79, 142), "step of 63")


@pytest.mark.parametrize("h,kvh,d", [(129, 129, 128), (18, 2, 128)])  # h*d = 16512 > 16384; h / kvh = 9 > 8
def test_shapes_outside_the_contract_are_refused(dev, h, kvh, d):
    """QQQ_ERR_ARG with a message that names the entry, from the shape check in front of every launch.  Every buffer has the size the
    shape would need."""
    from qqq_amd import _lib

    L = _lib.lib()
    b, bs, cap = 2, 16, 32
    st = torch.cuda.current_stream().cuda_stream
    q = torch.zeros((b, h, 1, d), dtype=torch.float16, device=dev)
    o = torch.full((b, h * d), -1234.0, dtype=torch.float16, device=dev)
    xq = torch.full((b, h * d), 77, dtype=torch.int8, device=dev)
    s1 = torch.full((b, 1), -1234.0, dtype=torch.float32, device=dev)
    ws = torch.zeros((b * h * (d + 2) * 4,), dtype=torch.uint8, device=dev)
    pos = torch.zeros(b, dtype=torch.int64, device=dev)
    cu = torch.arange(b + 1, dtype=torch.int32, device=dev)
    table = torch.arange(b * (cap // bs), dtype=torch.int32, device=dev).reshape(b, cap // bs)
    c16 = tuple(torch.zeros((b, kvh, cap, d), dtype=torch.float16, device=dev) for _ in range(2))
    c8 = tuple(torch.zeros((b, kvh, cap, d), dtype=torch.int8, device=dev) for _ in range(2)) + \
        tuple(torch.ones((b, kvh, cap), dtype=torch.float32, device=dev) for _ in range(2))
    p = lambda ts: tuple(t.data_ptr() for t in ts)
    out = (o.data_ptr(), xq.data_ptr(), s1.data_ptr())
    nb = b * (cap // bs)  # the contiguous caches, read as pools of nb blocks of bs slots
    assert L.qqq_decode_attn_workspace_bytes(b, h, kvh, d, cap) == 0 and L.qqq_prefill_attn_workspace_bytes(b, h, d) in (0, b * h * d * 2)
    calls = {
        "qqq_decode_attn": lambda: L.qqq_decode_attn(q.data_ptr(), *p(c16), pos.data_ptr(), d ** -0.5, *out, ws.data_ptr(), ws.numel(), b, h, kvh,
                                                     d, cap, cap, 0, st),
        "qqq_decode_attn_kv8": lambda: L.qqq_decode_attn_kv8(q.data_ptr(), *p(c8), pos.data_ptr(), d ** -0.5, *out, ws.data_ptr(), ws.numel(), b,
                                                             h, kvh, d, cap, cap, 0, st),
        "qqq_decode_attn_paged": lambda: L.qqq_decode_attn_paged(q.data_ptr(), *p(c16), table.data_ptr(), table.shape[1], pos.data_ptr(),
                                                                 d ** -0.5, *out, ws.data_ptr(), ws.numel(), b, h, kvh, d, nb, bs, cap, 0, st),
        "qqq_decode_attn_paged_kv8": lambda: L.qqq_decode_attn_paged_kv8(q.data_ptr(), *p(c8), table.data_ptr(), table.shape[1], pos.data_ptr(),
                                                                         d ** -0.5, *out, ws.data_ptr(), ws.numel(), b, h, kvh, d, nb, bs, cap, 0,
                                                                         st),
        "qqq_prefill_attn_paged": lambda: L.qqq_prefill_attn_paged(q.data_ptr(), *p(c16), table.data_ptr(), table.shape[1], cu.data_ptr(),
                                                                   pos.data_ptr(), d ** -0.5, *out, ws.data_ptr(), ws.numel(), b, b, h, kvh, d, nb,
                                                                   bs, cap, 0, st),
        "qqq_prefill_attn_paged_kv8": lambda: L.qqq_prefill_attn_paged_kv8(q.data_ptr(), *p(c8), table.data_ptr(), table.shape[1], cu.data_ptr(),
                                                                           pos.data_ptr(), d ** -0.5, *out, ws.data_ptr(), ws.numel(), b, b, h,
                                                                           kvh, d, nb, bs, cap, 0, st),
    }
    for name, call in calls.items():
        err = call()
        msg = _lib.last_error()
        assert err == ERR_ARG and msg.startswith(name + ": bad shape"), (name, err, msg)
    torch.cuda.synchronize()
    assert bool((o == -1234.0).all()) and bool((xq == 77).all()) and bool((s1 == -1234.0).all())  # nothing ran
