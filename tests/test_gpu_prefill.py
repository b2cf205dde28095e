"""The paged prefill attention on the GPU (include/qqq_amd_prefill.h): ragged packed steps against float64 attention, a peaked softmax, the
bit-exact invariances (block size and table permutation, batch composition, chunking, a shared prefix), rows that write nothing, a decode
row against decode_attention_paged, hipGraph replay with the step's metadata updated in place, torch.compile, and the decoder layer with
fuse_prefill() against every sequence run alone on a contiguous cache.

Every pool is reached through a random permutation of its blocks; every table entry beyond a row's need names a poison block (NaN for fp16;
codes 127 with NaN scales for int8) and the slots of a sequence's last block beyond its last key are poisoned too, so any read outside a
sequence's keys shows up as NaN."""
import pytest
import torch
import torch.nn.functional as F

import kv8_ref as K8
from test_gpu_attn import _bits, _make_layer, _tables
from test_gpu_paged import SENT, SHAPES, _i32, _raw, _rel, _shuffled_table, _to_pool

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _cont(dev, g, lens, kvh, d, cap, kv8, amp=1.0):
    """contiguous caches [b, kvh, cap, d] with random rows; fp16 (k, v) or int8 (k, v, k_scale, v_scale)"""
    b = len(lens)
    k = (torch.randn((b, kvh, cap, d), generator=g, device=dev) * amp).half()
    v = torch.randn((b, kvh, cap, d), generator=g, device=dev).half()
    if kv8:
        kc, ks = K8.quant_rows_op(k)
        vc, vs = K8.quant_rows_op(v)
        return (kc, vc, ks, vs)
    return (k, v)


def _pools(g, cont, lens, bs, kv8):
    """(pools, int32 table [b, W]) holding the rows of `cont` below each sequence's length; everything else is poison"""
    b, _, cap = cont[0].shape[:3]
    dev = cont[0].device
    table, nb, spare = _shuffled_table(g, b, cap // bs, dev, spare=1)
    fills = (127, 127, NAN, NAN) if kv8 else (NAN, NAN)
    pools = []
    for t, fill in zip(cont, fills):
        t = t.clone()
        for i, n in enumerate(lens):
            t[i, :, n:] = fill  # the slots beyond a sequence's last key, its last block's included
        pools.append(_to_pool(t, table, nb, fill))
    need = torch.tensor([-(-n // bs) for n in lens], device=dev)[:, None]
    cols = torch.arange(cap // bs, device=dev)[None]
    tab = torch.where(cols < need, table, torch.full_like(table, int(spare[0]))).to(torch.int32)
    return tuple(pools), tab


def _meta(dev, seqs):
    cu = [0]
    for _, c in seqs:
        cu.append(cu[-1] + c)
    return (torch.tensor(cu, dtype=torch.int32, device=dev), torch.tensor([s for s, _ in seqs], dtype=torch.int64, device=dev))


def _run(q, pools, table, cu, sp, scale, kv8, max_len=None):
    from qqq_amd import ops

    fn = ops.prefill_attention_paged_kv8 if kv8 else ops.prefill_attention_paged
    out = fn(q, *pools, table, cu, sp, scale, max_len=max_len, return_fp16=True)
    torch.cuda.synchronize()
    return out  # (xq, s1, o_fp16)


def _kv64(cont, kv8):
    if kv8:
        return K8.dequant64(cont[0], cont[2]), K8.dequant64(cont[1], cont[3])
    return cont[0].double(), cont[1].double()


def _ref64(q, k64, v64, seqs, scale):
    """float64 causal attention of the packed tokens q [m, h, d]: (out [m, h, d], max |v| over the keys each (token, head) attends [m, h])"""
    m, h, d = sum(c for _, c in seqs), q.shape[1], q.shape[2]
    kvh = k64.shape[1]
    out = torch.empty((m, h, d), dtype=torch.float64, device=q.device)
    vmax = torch.empty((m, h), dtype=torch.float64, device=q.device)
    t = 0
    for i, (start, c) in enumerate(seqs):
        n = start + c
        k = k64[i, :, :n].repeat_interleave(h // kvh, 0)
        v = v64[i, :, :n].repeat_interleave(h // kvh, 0)
        s = torch.einsum("thd,hkd->htk", q[t:t + c].double(), k) * scale
        keep = torch.arange(n, device=q.device)[None] <= (start + torch.arange(c, device=q.device))[:, None]
        s = s.masked_fill(~keep[None], -float("inf"))
        out[t:t + c] = torch.einsum("htk,hkd->thd", torch.softmax(s, -1), v)
        vmax[t:t + c] = torch.cummax(v64[i, :, :n].abs().amax(dim=2), 1).values[:, start:n].t().repeat_interleave(h // kvh, 1)
        t += c
    return out, vmax


def _sdpa(q, k16, v16, seqs, scale):
    """torch's attention over the contiguous copy, per sequence: what the unfused module path computes"""
    h, kvh = q.shape[1], k16.shape[1]
    outs, t = [], 0
    for i, (start, c) in enumerate(seqs):
        n = start + c
        mask = torch.ones((c, n), dtype=torch.bool, device=q.device).tril(diagonal=start)
        o = F.scaled_dot_product_attention(q[t:t + c].transpose(0, 1)[None], k16[i:i + 1, :, :n], v16[i:i + 1, :, :n], attn_mask=mask,
                                           scale=scale, enable_gqa=h != kvh)
        outs.append(o[0].transpose(0, 1))
        t += c
    return torch.cat(outs)


def _errors(o, ref, vmax):
    """(worst relative L2 per (token, head), worst max |o - ref| / max |v| over the keys the token attends)"""
    o = o.double().reshape(ref.shape)
    rel = ((o - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)).max().item()
    return rel, ((o - ref).abs().amax(dim=2) / vmax).max().item()


def _assert_quant(xq, s1, o, rows, what):
    from qqq_amd import ops

    wq, ws = ops.dynamic_quant(o[:rows].contiguous())
    assert torch.equal(xq[:rows], wq) and torch.equal(_i32(s1[:rows]), _i32(ws)), what


STEP = [(0, 1), (0, 133), (13, 65), (250, 64), (1000, 17), (300, 1)]
PAD = 3


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("bs", [16, 32, 128])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,kvh", SHAPES)
def test_packed_step_against_float64(dev, d, h, kvh, bs, kv8):
    """relative L2 per (token, head) <= 1e-3 and max error <= 2^-9 max|v| over the keys attended: the bounds of tests/test_gpu_decode_attn.py
    and tests/test_gpu_kv8.py for this arithmetic (int8: against float64 attention over the dequantised pool)."""
    g = torch.Generator(device=dev).manual_seed(h * 5 + kvh + d + bs)
    lens = [s + c for s, c in STEP]
    cont = _cont(dev, g, lens, kvh, d, 1024, kv8)
    pools, table = _pools(g, cont, lens, bs, kv8)
    m = sum(c for _, c in STEP)
    q = torch.randn((m + PAD, h, d), generator=g, device=dev).half()
    cu, sp = _meta(dev, STEP)
    xq, s1, o = _run(q, pools, table, cu, sp, d ** -0.5, kv8)
    assert xq.shape == (m + PAD, h * d) and s1.shape == (m + PAD, 1) and o.shape == (m + PAD, h * d)
    assert torch.isfinite(o[:m].float()).all() and torch.isfinite(s1[:m]).all()
    k64, v64 = _kv64(cont, kv8)
    ref, vmax = _ref64(q, k64, v64, STEP, d ** -0.5)
    rel, mx = _errors(o[:m], ref, vmax)
    srel, smx = _errors(_sdpa(q, k64.half(), v64.half(), STEP, d ** -0.5), ref, vmax)
    print(f"prefill_attention_paged{'_kv8' if kv8 else ''} h={h} kvh={kvh} d={d} bs={bs}: rel L2 {rel:.2e}, max|err|/max|v| {mx:.2e} "
          f"(2^-9 = {2 ** -9:.2e});  SDPA over the gathered copy {srel:.2e}, {smx:.2e}")
    assert rel <= 1e-3 and mx <= 2 ** -9, (rel, mx)
    _assert_quant(xq, s1, o, m, (d, h, kvh, bs, kv8))


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("where", ["first tile", "diagonal tile", "own key"])
def test_peaked_softmax(dev, where, kv8):
    """one key whose score exceeds every other by more than 100 (log2 domain included): in the first key tile, in the diagonal tile, and as
    the token's own key"""
    h, kvh, d, bs = 32, 8, 128, 16
    seqs = [(150, 70)]
    g = torch.Generator(device=dev).manual_seed(77)
    cont = [t.clone() for t in _cont(dev, g, [220], kvh, d, 256, False, amp=0.25)]
    q = (torch.randn((70, h, d), generator=g, device=dev) * 0.25).half()
    tok = 40  # the token under test sits at position 190
    peak = {"first tile": 3, "diagonal tile": 185, "own key": 190}[where]
    unit = torch.zeros(d, device=dev)
    unit[::2] = 1.0
    q[tok] = (unit * 4).half()  # the peaked key scores 4 * 4 * 64 * 1.5 * d^-0.5 = 136, every other key (scaled by 0.05) stays below 1
    cont[0][0, :, peak] = (unit * 4).half()
    cont[0][0, :, :peak] *= 0.05
    cont[0][0, :, peak + 1:] *= 0.05
    cont = tuple(cont)
    if kv8:
        kc, ks = K8.quant_rows_op(cont[0])
        vc, vs = K8.quant_rows_op(cont[1])
        cont = (kc, vc, ks, vs)
    pools, table = _pools(g, cont, [220], bs, kv8)
    cu, sp = _meta(dev, seqs)
    xq, s1, o = _run(q, pools, table, cu, sp, d ** -0.5 * 1.5, kv8)
    k64, v64 = _kv64(cont, kv8)
    scale = d ** -0.5 * 1.5
    s = torch.einsum("hd,hkd->hk", q[tok].double(), k64[0, :, :191].repeat_interleave(h // kvh, 0)) * scale
    gap = (s[:, peak:peak + 1] - torch.cat([s[:, :peak], s[:, peak + 1:]], 1)).min().item()
    assert gap > 100, gap
    ref, vmax = _ref64(q, k64, v64, seqs, scale)
    rel, mx = _errors(o, ref, vmax)
    print(f"peaked softmax ({where}, kv8={kv8}): score gap {gap:.1f}, rel L2 {rel:.2e}, max|err|/max|v| {mx:.2e}")
    assert torch.isfinite(o.float()).all() and rel <= 1e-3 and mx <= 2 ** -9, (rel, mx)
    _assert_quant(xq, s1, o, 70, where)


def _same(a, b, rows_a, rows_b, what):
    for name, x, y in zip(("xq", "s1", "o_fp16"), a, b):
        assert torch.equal(_raw(x[rows_a]), _raw(y[rows_b])), (what, name)


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("h,kvh,d", [(32, 8, 128), (28, 4, 64), (32, 32, 128)])
def test_bit_exact_invariances(dev, h, kvh, d, kv8):
    """o_fp16, xq and s1 of a token depend on its query, position and keys only: not on the block size or the table, not on the rest of the
    batch, not on how its sequence is cut into steps, not on whether its first blocks are shared with another row"""
    g = torch.Generator(device=dev).manual_seed(h + kvh + d)
    seqs = [(40, 9), (0, 133), (77, 50)]
    lens = [s + c for s, c in seqs]
    cont = _cont(dev, g, lens, kvh, d, 256, kv8)
    cont = tuple(t.clone() for t in cont)
    for t in cont:
        t[2, :, :64] = t[1, :, :64]  # rows 1 and 2 hold the same first 64 keys
    m = sum(c for _, c in seqs)
    q = torch.randn((m, h, d), generator=g, device=dev).half()
    cu, sp = _meta(dev, seqs)
    scale = d ** -0.5
    base = None
    for bs in (16, 32, 128):
        pools, table = _pools(g, cont, lens, bs, kv8)
        out = _run(q, pools, table, cu, sp, scale, kv8)
        assert torch.isfinite(out[2].float()).all()
        if base is None:
            base, base_pools, base_table = out, pools, table
        else:
            _same(out, base, slice(None), slice(None), f"block_size {bs}")
    pools, table = base_pools, base_table  # block_size 16
    # a sequence alone against the same sequence as second of three
    cu1, sp1 = _meta(dev, seqs[1:2])
    alone = _run(q[9:142].contiguous(), pools, table[1:2], cu1, sp1, scale, kv8)
    _same(alone, base, slice(None), slice(9, 142), "alone")
    # 133 tokens in one step against steps of 70 and 63 (all 133 keys are in the pool; the first step must not see the later ones)
    cu_a, sp_a = _meta(dev, [(0, 70)])
    cu_b, sp_b = _meta(dev, [(70, 63)])
    first = _run(q[9:79].contiguous(), pools, table[1:2], cu_a, sp_a, scale, kv8)
    second = _run(q[79:142].contiguous(), pools, table[1:2], cu_b, sp_b, scale, kv8)
    _same(first, base, slice(None), slice(9, 79), "step of 70")
    _same(second, base, slice(None), slice(79, 142), "step of 63")
    # rows 1 and 2 share their first 64 keys: row 2 names row 1's blocks for them
    shared = table.clone()
    shared[2, :4] = table[1, :4]
    out = _run(q, pools, shared, cu, sp, scale, kv8)
    _same(out, base, slice(None), slice(None), "shared prefix")


@pytest.mark.parametrize("kv8", [False, True])
def test_rows_that_write_nothing(dev, kv8):
    from qqq_amd import _lib

    h, kvh, d, bs, cap, max_len = 32, 8, 128, 32, 512, 300
    g = torch.Generator(device=dev).manual_seed(29)
    #        negative start   fits     ends past max_len   reads a corrupt table entry
    seqs = [(-1, 20), (270, 30), (280, 21), (10, 70)]
    lens = [64, 300, 301, 80]
    cont = _cont(dev, g, lens, kvh, d, cap, kv8)
    pools, table = _pools(g, cont, lens, bs, kv8)
    for t, fill in zip(pools, (1, 1, 0.01, 0.01) if kv8 else (0.5, 0.5)):
        t[-1] = fill  # the block a too large id is clamped to holds finite rows, whoever owns it
    saved = [t.clone() for t in pools]
    table[0], table[2] = -7, 1 << 30  # rows that are never read
    good = table.clone()
    table[3, 1] = 1 << 30  # read (keys 32 ... 63 of row 3): clamped into the pool
    m, pad = sum(c for _, c in seqs), 5
    q = torch.randn((m + pad, h, d), generator=g, device=dev).half()
    cu, sp = _meta(dev, seqs)
    o = torch.full((m + pad, h * d), SENT, dtype=torch.float16, device=dev)
    xq = torch.full((m + pad, h * d), 77, dtype=torch.int8, device=dev)
    s1 = torch.full((m + pad, 1), SENT, dtype=torch.float32, device=dev)
    L = _lib.lib()
    fn = L.qqq_prefill_attn_paged_kv8 if kv8 else L.qqq_prefill_attn_paged
    err = fn(q.data_ptr(), *(t.data_ptr() for t in pools), table.data_ptr(), table.shape[1], cu.data_ptr(), sp.data_ptr(), d ** -0.5,
             o.data_ptr(), xq.data_ptr(), s1.data_ptr(), None, 0, m + pad, len(seqs), h, kvh, d, pools[0].shape[0], bs, max_len, 0,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert err == 0, _lib.last_error()
    dead = torch.ones(m + pad, dtype=torch.bool, device=dev)
    dead[20:50] = False
    dead[71:141] = False
    assert bool((o[dead] == SENT).all()) and bool((xq[dead] == 77).all()) and bool((s1[dead] == SENT).all())
    for t, t0 in zip(pools, saved):
        assert torch.equal(_raw(t), _raw(t0))  # the pools are only read
    assert torch.isfinite(o[~dead].float()).all() and torch.isfinite(s1[~dead]).all()  # the corrupt entry gives finite output
    want = _run(q, pools, good, cu, sp, d ** -0.5, kv8, max_len=max_len)
    _same((xq, s1, o), want, slice(20, 50), slice(20, 50), "the sequence that fits")
    if int(good[3, 1]) != pools[0].shape[0] - 1:
        assert not torch.equal(_raw(o[71:141]), _raw(want[2][71:141]))  # the clamped block is another one
    # the same call without o_fp16: the rows go through the workspace
    nbytes = L.qqq_prefill_attn_workspace_bytes(m + pad, h, d)
    assert nbytes == (m + pad) * h * d * 2
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    xq2, s12 = torch.full_like(xq, 77), torch.full_like(s1, SENT)
    err = fn(q.data_ptr(), *(t.data_ptr() for t in pools), table.data_ptr(), table.shape[1], cu.data_ptr(), sp.data_ptr(), d ** -0.5,
             None, xq2.data_ptr(), s12.data_ptr(), ws.data_ptr(), nbytes, m + pad, len(seqs), h, kvh, d, pools[0].shape[0], bs, max_len, 0,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert err == 0, _lib.last_error()
    assert torch.equal(xq2, xq) and torch.equal(_i32(s12), _i32(s1))


@pytest.mark.parametrize("kv8", [False, True])
def test_decode_row_against_decode_attention_paged(dev, kv8):
    """a one-token row at position 2077: the decode kernel splits the keys and the prefill kernel does not, so relative L2 <= 1e-2, the
    project's bound between decode paths"""
    from qqq_amd import ops

    h, kvh, d, bs, cap = 32, 8, 128, 16, 2176
    g = torch.Generator(device=dev).manual_seed(2077)
    cont = _cont(dev, g, [2078], kvh, d, cap, kv8)
    pools, table = _pools(g, cont, [2078], bs, kv8)
    q = torch.randn((1, h, d), generator=g, device=dev).half()
    cu, sp = _meta(dev, [(2077, 1)])
    xq, s1, o = _run(q, pools, table, cu, sp, d ** -0.5, kv8)
    dec = ops.decode_attention_paged_kv8 if kv8 else ops.decode_attention_paged
    want = dec(q, *pools, table, sp, d ** -0.5, return_fp16=True)[2]
    rel = _rel(o, want)
    print(f"decode row at 2077 (kv8={kv8}): relative L2 vs decode_attention_paged {rel:.2e}")
    assert torch.isfinite(o.float()).all() and rel <= 1e-2, rel
    _assert_quant(xq, s1, o, 1, "decode row")


@pytest.mark.parametrize("kv8", [False, True])
def test_hipgraph_replays_with_the_step_updated_in_place(dev, kv8):
    from qqq_amd import PagedKVCache, ops

    h, kvh, d, bs, width, nb = 32, 8, 128, 16, 16, 40
    m, b = 48, 3
    dtype = torch.int8 if kv8 else torch.float16
    cos, sin = _tables(dev, width * bs, d, seed=6)
    g = torch.Generator(device=dev).manual_seed(43)
    write = ops.rope_qkv_paged_kv8 if kv8 else ops.rope_qkv_paged
    prefill = ops.prefill_attention_paged_kv8 if kv8 else ops.prefill_attention_paged
    nq, nk = h * d, kvh * d

    def pools_of(c):
        return (c.k[0], c.v[0]) + ((c.k_scale[0], c.v_scale[0]) if kv8 else ())

    def step(qkv, pos, slots, table, cu, sp, pools):
        q_out = write(qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:], cos, sin, pos, slots, *pools)
        return (q_out,) + tuple(prefill(q_out, *pools, table, cu, sp, d ** -0.5, max_len=width * bs, return_fp16=True))

    cg, ce = (PagedKVCache(1, nb, kvh, d, bs, dev, dtype=dtype) for _ in range(2))  # the graph's pools and the eager call's: same allocator
    for c in (cg, ce):
        for sid in range(b):
            c.add(sid)
    qkv = torch.randn((m, (h + 2 * kvh) * d), generator=g, device=dev).half()
    pos = torch.zeros(m, dtype=torch.int64, device=dev)
    slots = torch.full((m,), -1, dtype=torch.int64, device=dev)  # the warm-up and the capture write no cache row
    table = torch.zeros((b, width), dtype=torch.int32, device=dev)
    cu = torch.zeros(b + 1, dtype=torch.int32, device=dev)  # ... and attend nothing: every token is padding
    sp = torch.zeros(b, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(qkv, pos, slots, table, cu, sp, pools_of(cg))  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = step(qkv, pos, slots, table, cu, sp, pools_of(cg))
    torch.cuda.current_stream().wait_stream(side)
    assert all(not t.any() for t in pools_of(cg))
    for it, counts in enumerate([(20, 20, 5), (1, 25, 22), (30, 1, 12)]):  # other splits of m over the sequences, 3 / 0 / 5 padding tokens
        sg, se = cg.step(range(b), counts), ce.step(range(b), counts)
        n = sum(counts)
        assert torch.equal(sg.slots, se.slots) and torch.equal(sg.block_table, se.block_table)
        pos.zero_()
        pos[:n] = sg.pos
        slots.fill_(-1)
        slots[:n] = sg.slots
        table.zero_()
        table[:, :sg.block_table.shape[1]] = sg.block_table
        cu.copy_(sg.cu_tokens)
        sp.copy_(sg.start_pos)
        qkv.copy_(torch.randn(qkv.shape, generator=g, device=dev).half())
        graph.replay()
        torch.cuda.synchronize()
        want = step(qkv, pos, slots, table, cu, sp, pools_of(ce))
        torch.cuda.synchronize()
        assert torch.equal(_bits(out[0]), _bits(want[0])), (kv8, it)
        for g_, w_ in zip(out[1:], want[1:]):
            assert torch.equal(_raw(g_[:n]), _raw(w_[:n])), (kv8, it)
        assert torch.isfinite(out[3][:n].float()).all()
        for t_, e_ in zip(pools_of(cg), pools_of(ce)):
            assert torch.equal(_raw(t_), _raw(e_)), (kv8, it)
    assert cg.length(1) == 46 and len(cg.blocks(1)) == 3


def test_prefill_ops_trace_under_torch_compile(dev):
    from qqq_amd import ops

    h, kvh, d, bs = 28, 4, 128, 32
    seqs = [(5, 40), (100, 1), (0, 37)]
    lens = [s + c for s, c in seqs]
    g = torch.Generator(device=dev).manual_seed(10)
    c16 = _cont(dev, g, lens, kvh, d, 128, False)
    c8 = _cont(dev, g, lens, kvh, d, 128, True)
    p16, table = _pools(g, c16, lens, bs, False)
    p8, table8 = _pools(g, c8, lens, bs, True)
    m = sum(c for _, c in seqs)
    q = torch.randn((m, h, d), generator=g, device=dev).half()
    cu, sp = _meta(dev, seqs)

    def f(q, k16, v16, k8, v8, ks, vs, table, table8, cu, sp):
        xq, s1, o = ops.prefill_attention_paged(q * 1, k16, v16, table, cu, sp, d ** -0.5, return_fp16=True)
        xq8, s18 = ops.prefill_attention_paged_kv8(q * 1, k8, v8, ks, vs, table8, cu, sp, d ** -0.5, max_len=128)
        return xq, s1 * 2, o, xq8, s18 * 2

    eager = f(q, *p16, *p8, table, table8, cu, sp)
    comp = torch.compile(f, fullgraph=True)(q, *p16, *p8, table, table8, cu, sp)
    for e, c in zip(eager, comp):
        assert torch.equal(_raw(e), _raw(c))


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_layer_with_fuse_prefill(dev, dtype):
    """Packed prefill of 5, 70 and 133 tokens, a mixed step of a 24-token chunk and two decoding rows, three decode steps: every sequence
    against the same layer run alone on KVCache(batch=1) within relative L2 1e-2 (the project's bound between attention paths), the cache
    rows bit for bit, and the whole against the unfused paged layer within 1e-2."""
    from qqq_amd import KVCache, PagedKVCache

    hidden, heads, kvh, inter = 1024, 8, 2, 2048
    layer = _make_layer(dev, hidden, heads, kvh, inter, 128, False, seed=63).eval()
    keys = sorted(layer.state_dict())
    assert not layer.prefill_fused and not layer.self_attn.prefill_fused
    d, bs = hidden // heads, 16
    pre = {"a": 5, "b": 70, "c": 133}
    plan = [(["a", "b", "c"], [5, 70, 133]), (["a", "b", "c"], [24, 1, 1])] + [(["a", "b", "c"], [1, 1, 1])] * 3
    total = {sid: sum(c[sids.index(sid)] for sids, c in plan) for sid in pre}
    g = torch.Generator(device=dev).manual_seed(8)
    xs = {sid: torch.randn((n, hidden), generator=g, device=dev).half() for sid, n in total.items()}

    def run_paged():
        paged = PagedKVCache(1, 2 + 5 + 9 + 1, kvh, d, bs, dev, dtype=dtype)
        for sid in pre:
            paged.add(sid)
        got, done = {sid: [] for sid in pre}, {sid: 0 for sid in pre}
        for sids, counts in plan:
            st = paged.step(sids, counts)
            assert st.cu_tokens.dtype == torch.int32 and st.start_pos.dtype == torch.int64 and st.cu_tokens.is_cuda
            x = torch.cat([xs[s][done[s]:done[s] + c] for s, c in zip(sids, counts)])
            out = layer(x, paged, st)
            assert torch.isfinite(out).all()
            t = 0
            for s, c in zip(sids, counts):
                got[s].append(out[t:t + c])
                done[s] += c
                t += c
        return paged, got

    _, unfused = run_paged()
    assert layer.fuse_prefill() is layer and layer.prefill_fused and layer.self_attn.prefill_fused
    assert sorted(layer.state_dict()) == keys
    paged, got = run_paged()
    worst = 0.0
    for sid, n in total.items():
        alone = KVCache(1, 1, kvh, d, 160, dev, dtype=dtype)
        want, t = [], 0
        for sids, counts in plan:
            c = counts[sids.index(sid)]
            want.append(layer(xs[sid][None, t:t + c], alone, t)[0])
            t += c
        for i, (g_, w_, u_) in enumerate(zip(got[sid], want, unfused[sid])):
            rel, relu = _rel(g_, w_), _rel(g_, u_)
            worst = max(worst, rel, relu)
            assert rel <= 1e-2 and relu <= 1e-2, (dtype, sid, i, rel, relu)
        kg, vg = paged.gather(0, sid)
        kc, vc = alone.dequant(0, n) if dtype == torch.int8 else (alone.k[0][:, :, :n], alone.v[0][:, :, :n])
        assert torch.equal(_bits(kg), _bits(kc)) and torch.equal(_bits(vg), _bits(vc)), sid
    print(f"fuse_prefill layer ({dtype}): worst relative L2 vs each sequence alone and vs the unfused paged layer {worst:.2e}")
    assert layer.unfuse_prefill() is layer and not layer.prefill_fused
