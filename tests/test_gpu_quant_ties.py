"""Every copy of the per-row int8 quantiser on the GPU at the inputs where its shortcut needs its fallback (tests/quant_ref.py): the rows of
corpus(L) hold every exact tie x / s1 = n + 1/2 at which rint(x * (1 / s1)) is the wrong integer, in both signs, for all 880 scales that
have one, and edge_rows(L) the ends of the format (zero scale, the clamp, fp16 max).  Each kernel is given input from which it forms
exactly these rows, and its (xq, s1) must be quant_ref.quant_rows_exact of the fp16 row it quantised, bit for bit:

    qqq_dynamic_quant_kernel        dynamic_quant of the rows themselves, all six launch-ladder instantiations
    qqq_kv8_quant_head_row          rope_qkv_kv8 / rope_qkv_paged_kv8 with the rows as V head rows and, under cos = 1, sin = 0, as K head rows
    qqq_act_quant_row               decode_attention (contiguous and paged) at pos 0 and prefill_attention_paged with one-token sequences:
                                    with one key the output is the V row; silu_mul_quant with gate = 32, up = row / 32; rmsnorm_quant with
                                    x = +-1 and the row as weight

A test asserts that the row a kernel quantised is the crafted one wherever it can see that row, and counts the hard ties in it."""
import numpy as np
import pytest
import torch

import quant_ref as Q
from test_gpu_paged import _from_pool, _shuffled_table, _slots, _to_pool

pytestmark = pytest.mark.gpu

N_HARD = 2 * 3824  # distinct (scale, x) hard ties, both signs


def _i32(t):
    return t.contiguous().view(torch.int32)


def _with_edges(L):
    return np.concatenate([Q.corpus(L).rows, Q.edge_rows(L)])


def _reference(y):
    """quant_rows_hard of a torch fp16 tensor's last-dim rows: numpy (codes [m, k], scales [m, 1], hard-tie mask [m, k], the rows)"""
    yn = y.detach().cpu().numpy().reshape(-1, y.shape[-1])
    return Q.quant_rows_hard(yn) + (yn,)


def _assert_codes(xq, s1, ref, what):
    q, s, hard, _ = ref
    got_s = s1.detach().cpu().numpy().reshape(-1, 1)
    assert np.array_equal(got_s.view(np.uint32), s.view(np.uint32)), (what, "scales", int((got_s != s).sum()))
    bad = xq.detach().cpu().numpy().reshape(q.shape) != q
    assert not bad.any(), (what, f"{int(bad.sum())} codes differ, {int((bad & hard).sum())} of them at hard ties, first at {np.argwhere(bad)[0]}")


def _distinct_hard(ref):
    return len(Q.hard_tie_keys(ref[3], ref[2]))


# ---- qqq_dynamic_quant_kernel

@pytest.mark.parametrize("k", [8, 64, 4096, 4104, 8192, 16384, 16392, 32768, 32776, 65536])
def test_dynamic_quant_on_the_corpus(dev, k):
    """One call with all rows (m > 512) and calls of at most 512 rows: with these k the two reach <2,256> <4,256> <8,256> and <2,1024>
    <4,1024> <8,1024> of the launch ladder."""
    from oracle import c_oracle as C
    from qqq_amd import ops

    rows = _with_edges(k)
    m = len(rows)
    assert m > 512
    y = torch.from_numpy(rows).to(dev)
    ref = _reference(y)
    q, s, hard, _ = ref
    assert _distinct_hard(ref) == N_HARD and int((s == 0).sum()) == 3
    xq, s1 = ops.dynamic_quant(y)
    _assert_codes(xq, s1, ref, f"k={k} m={m}")
    step = -(-m // -(-m // 512))
    for a in range(0, m, step):
        part = ops.dynamic_quant(y[a:a + step])
        assert torch.equal(part[0], xq[a:a + step]) and torch.equal(_i32(part[1]), _i32(s1[a:a + step])), (k, a)
    # the oracle and the reference expression as torch evaluates it on this GPU divide by the scale: rows with a scale above zero
    live = s[:, 0] > 0
    oq, os1 = C.dynamic_quant(rows[live], "recip")
    assert np.array_equal(os1.view(np.uint32), s[live].view(np.uint32)) and np.array_equal(oq, q[live])
    lt = torch.from_numpy(live).to(dev)
    ts = y[lt].abs().max(dim=-1, keepdim=True)[0].div(127.0).to(torch.float32)
    tq = (y[lt] / ts).round().clamp(-128, 127).to(torch.int8)
    assert torch.equal(_i32(ts), _i32(s1[lt])) and torch.equal(tq, xq[lt]), k
    print(f"dynamic_quant k={k}: {m} rows, {int(hard.sum())} hard ties ({N_HARD} distinct)")


# ---- qqq_kv8_quant_head_row

@pytest.mark.parametrize("d", [64, 128])
def test_rope_qkv_kv8_on_the_corpus(dev, d):
    """The rows as V head rows and, rolled by one row, as K head rows under the identity rotation (cos = 1, sin = 0): the fp16 ops must
    cache exactly the crafted rows, the int8 ops their exact quantisation."""
    from qqq_amd import ops

    h, kvh, bs = 16, 8, 16
    rows = _with_edges(d)
    m = -(-len(rows) // kvh)
    cap = -(-m // bs) * bs
    pad = np.zeros((m * kvh - len(rows), d), np.float16)
    vrows = torch.from_numpy(np.concatenate([rows, pad])).to(dev)
    krows = vrows.roll(1, 0)
    g = torch.Generator(device=dev).manual_seed(d)
    q = torch.randn((m, h * d), generator=g, device=dev).half()
    k, v = krows.reshape(m, kvh * d), vrows.reshape(m, kvh * d)
    cos, sin = torch.ones((cap, d), dtype=torch.float16, device=dev), torch.zeros((cap, d), dtype=torch.float16, device=dev)
    pos = torch.arange(m, device=dev)
    want = tuple(t.reshape(m, kvh, d).transpose(0, 1)[None] for t in (krows, vrows))  # [1, kvh, m, d]

    def check(caches16, caches8, what):
        refs = []
        for c16, w in zip(caches16, want):
            assert torch.equal(c16[:, :, :m], w), (what, "the fp16 op did not cache the crafted rows")
            refs.append(_reference(c16[:, :, :m]))
        for (codes, scales), ref in zip(caches8, refs):
            _assert_codes(codes[:, :, :m], scales[:, :, :m], ref, what)
        assert _distinct_hard(refs[1]) == N_HARD and int(refs[0][2].sum()) == int(refs[1][2].sum()) == int(Q.hard_tie_mask(rows).sum())
        return int(refs[1][2].sum())

    kc16 = torch.full((1, kvh, cap, d), -1234.0, dtype=torch.float16, device=dev)
    vc16 = kc16.clone()
    ops.rope_qkv(q, k, v, cos, sin, pos, kc16, vc16)
    kc = torch.full((1, kvh, cap, d), 77, dtype=torch.int8, device=dev)
    ks = torch.full((1, kvh, cap), -1234.0, dtype=torch.float32, device=dev)
    vc, vs = kc.clone(), ks.clone()
    ops.rope_qkv_kv8(q, k, v, cos, sin, pos, kc, vc, ks, vs)
    n = check((kc16, vc16), ((kc, ks), (vc, vs)), f"rope_qkv_kv8 d={d}")
    # paged: the same rows through a shuffled block table
    table, nb, _ = _shuffled_table(g, 1, cap // bs, dev)
    slots = _slots(table, pos, 1, bs)
    kp16 = torch.full((nb, kvh, bs, d), -1234.0, dtype=torch.float16, device=dev)
    vp16 = kp16.clone()
    ops.rope_qkv_paged(q, k, v, cos, sin, pos, slots, kp16, vp16)
    kp = torch.full((nb, kvh, bs, d), 77, dtype=torch.int8, device=dev)
    ksp = torch.full((nb, kvh, bs), -1234.0, dtype=torch.float32, device=dev)
    vp, vsp = kp.clone(), ksp.clone()
    ops.rope_qkv_paged_kv8(q, k, v, cos, sin, pos, slots, kp, vp, ksp, vsp)
    gathered = lambda *ts: tuple(_from_pool(t, table) for t in ts)
    check(gathered(kp16, vp16), (gathered(kp, ksp), gathered(vp, vsp)), f"rope_qkv_paged_kv8 d={d}")
    print(f"rope_qkv_kv8 / rope_qkv_paged_kv8 d={d}: {len(rows)} head rows as K and as V, {n} hard ties each ({N_HARD} distinct)")


# ---- qqq_act_quant_row behind the attention kernels

@pytest.mark.parametrize("h,kvh,d", [(32, 8, 128), (64, 8, 128), (128, 16, 128)])  # VPT 1, 2 and 4 of the combine and the prefill quant kernel
def test_attention_over_one_key_on_the_corpus(dev, h, kvh, d):
    """With one key the probability is 1 and the sum 1, so o_fp16 is the V row with each head repeated h / kvh times (a -0 comes out as
    +0, the same code)."""
    from qqq_amd import ops

    G, bs = h // kvh, 16
    rows = _with_edges(kvh * d)
    b = len(rows)
    g = torch.Generator(device=dev).manual_seed(h)
    vrows = torch.from_numpy(rows).to(dev).reshape(b, kvh, d)
    want = vrows[:, :, None].expand(b, kvh, G, d).reshape(b, h * d)
    kc = torch.full((b, kvh, bs, d), float("nan"), dtype=torch.float16, device=dev)  # slots 1 ... 15 are never read
    vc = kc.clone()
    kc[:, :, 0] = torch.randn((b, kvh, d), generator=g, device=dev).half()
    vc[:, :, 0] = vrows
    q = torch.randn((b, h, 1, d), generator=g, device=dev).half()
    pos = torch.zeros(b, dtype=torch.int64, device=dev)
    n_rows = int(Q.hard_tie_mask(rows).sum())
    table, nb, _ = _shuffled_table(g, b, 1, dev)  # one block per row and a poison block
    pools = (_to_pool(kc, table, nb, float("nan")), _to_pool(vc, table, nb, float("nan")))
    tab = table.to(torch.int32)
    cu = torch.arange(b + 1, dtype=torch.int32, device=dev)
    calls = {"decode_attention": lambda: ops.decode_attention(q, kc, vc, pos, d ** -0.5, return_fp16=True),
             "decode_attention_paged": lambda: ops.decode_attention_paged(q, *pools, tab, pos, d ** -0.5, max_len=bs, return_fp16=True),
             "prefill_attention_paged": lambda: ops.prefill_attention_paged(q[:, :, 0], *pools, tab, cu, pos, d ** -0.5, max_len=bs,
                                                                           return_fp16=True)}
    for name, call in calls.items():
        xq, s1, o = call()
        torch.cuda.synchronize()
        ref = _reference(o)
        _assert_codes(xq, s1, ref, f"{name} h={h} kvh={kvh}")  # the contract, on the row that came back
        n = int(ref[2].sum())
        print(f"{name} h={h} kvh={kvh} d={d}: {b} rows, {n} hard ties in o_fp16 ({_distinct_hard(ref)} distinct)")
        assert torch.equal(o, want), (name, "o_fp16 is not the V row")
        assert n == G * n_rows and _distinct_hard(ref) == N_HARD, (name, n, n_rows)


# ---- qqq_act_quant_row behind silu_mul_quant and rmsnorm_quant: all six instantiations of the launch ladder

LADDER = {"2x256": (4096, True), "4x256": (8192, True), "8x256": (16384, True), "2x1024": (8192, False), "4x1024": (32768, False),
          "8x1024": (65536, False)}  # <VPT x NT>: (k, m > 512)


@pytest.mark.parametrize("inst", list(LADDER))
def test_silu_mul_quant_on_the_corpus(dev, inst):
    """gate = 32: 1 + expf(-32) is 1 in f32, so silu(gate) = 32 and y = fp16(32 * up) = row for up = row / 32, wherever row / 32 is exact in
    fp16: every value a multiple of 2^-19.  A row holds values down to half its scale, so these are the rows of the scales from 2^-8 up,
    578 of the 880."""
    from qqq_amd import ops

    k, big = LADDER[inst]
    c = Q.corpus(k)
    up_all = (c.rows.astype(np.float32) / 32).astype(np.float16)
    keep = (up_all.astype(np.float32) * 32 == c.rows).all(axis=1)
    rows, up_rows = c.rows[keep], up_all[keep]
    scales = Q.hard_ties().scales[c.scale_idx[keep]]
    assert np.array_equal(keep, Q.hard_ties().scales[c.scale_idx] >= 2.0 ** -8) and len(rows) == 578
    ref = Q.quant_rows_hard(rows) + (rows,)
    m = len(rows)
    step = m if big else 512
    gu = torch.empty((m, 2 * k), dtype=torch.float16, device=dev)
    gu[:, :k] = 32
    gu[:, k:] = torch.from_numpy(up_rows).to(dev)
    want = torch.from_numpy(rows).to(dev)
    outs = []
    for strided in (True, False):
        parts = []
        for a in range(0, m, step):
            gate, up = gu[a:a + step, :k], gu[a:a + step, k:]
            if not strided:
                gate, up = gate.contiguous(), up.contiguous()
            parts.append(ops.silu_mul_quant(gate, up, return_y=True))
            plain = ops.silu_mul_quant(gate, up)
            assert torch.equal(plain[0], parts[-1][0]) and torch.equal(_i32(plain[1]), _i32(parts[-1][1]))
        xq, s1, y = (torch.cat(t) for t in zip(*parts))
        assert torch.equal(y, want), (inst, strided, "y is not the crafted row")
        _assert_codes(xq, s1, ref, f"silu_mul_quant {inst} strided={strided}")
        outs.append((xq, s1))
    print(f"silu_mul_quant <{inst}> k={k}: {m} of {len(c.rows)} corpus rows are exactly divisible by 32 (scales {scales.min():.3e} ... "
          f"{scales.max():.1f}), {int(ref[2].sum())} hard ties ({_distinct_hard(ref)} distinct), calls of {step} rows")


def _spread_scales():
    """every 8th of the 880 scales that have a hard tie: 110 scales over every fp16 exponent field that has one, the subnormal included"""
    t = Q.hard_ties()
    hard_scales = np.unique(t.scale_idx[t.hard])
    pick = hard_scales[::8]
    field = lambda i: np.unique(t.scales[i].astype(np.float16).view(np.uint16) >> 10)
    assert len(pick) >= 100 and np.array_equal(field(pick), field(hard_scales)) and field(pick)[0] == 0
    return pick


@pytest.mark.parametrize("inst", list(LADDER))
def test_rmsnorm_quant_on_the_corpus(dev, inst):
    """x = +-1: the variance is 1, n = fp16(+-1 * rsqrt(1 + 1e-6)) = +-1, so y = +-weight, with four sign patterns over the rows.  One launch
    per scale and variant (residual or not, y stored or not); with the residual, h = fp16(2 sign - sign)."""
    from qqq_amd import ops

    k, big = LADDER[inst]
    m = 516 if big else 8
    c = Q.corpus(k)
    e = torch.arange(k, device=dev)
    signs = torch.stack([torch.ones(k, device=dev), -torch.ones(k, device=dev), 1.0 - 2.0 * (e % 2), 1.0 - 2.0 * ((e // 8 + e) % 3 == 0)]).half()
    rep = torch.arange(m, device=dev) % 4
    x = signs[rep].contiguous()
    total = distinct = 0
    for i in _spread_scales():
        w_np = c.rows[c.scale_idx == i][0]
        w = torch.from_numpy(w_np).to(dev)
        crafted = signs * w  # exact: +-1 times an fp16 value
        q, s, hard, _ = ref = _reference(crafted)
        total += int(hard.sum())
        distinct += _distinct_hard(ref)
        wq, ws = torch.from_numpy(q).to(dev)[rep], torch.from_numpy(s).to(dev)[rep]
        for with_res in (False, True):
            for return_y in (True, False):
                res = (2 * x) if with_res else None
                out = ops.rmsnorm_quant(-x if with_res else x, w, 1e-6, residual=res, return_y=return_y)
                what = (inst, int(i), with_res, return_y)
                if return_y:
                    assert torch.equal(out[2], crafted[rep]), (what, "y is not +-weight")
                if with_res:
                    assert torch.equal(res, x), what
                assert torch.equal(out[0], wq) and torch.equal(_i32(out[1]), _i32(ws)), what
    assert distinct >= 2 * 100  # at least one hard tie per scale, in both signs
    print(f"rmsnorm_quant <{inst}> k={k} m={m}: {len(_spread_scales())} scales, {distinct} distinct hard ties, {total} in the four sign patterns")
