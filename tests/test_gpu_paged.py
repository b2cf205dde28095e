"""The paged KV cache on the GPU (include/qqq_amd_paged.h).  The write ops bit for bit against rope_qkv / rope_qkv_kv8 into a contiguous
cache, the decode ops bit for bit against decode_attention / decode_attention_kv8 over a contiguous cache that holds the same rows (same b,
max_len and per-row pos), one float64 check per dtype that anchors the chain, hipGraph replay with pos / slots / block_table updated in
place, torch.compile, and the decoder layer over a PagedKVCache: uniform lengths against KVCache(batch=3), ragged lengths with a recycled
sequence against every sequence run alone."""
import pytest
import torch

import kv8_ref as K8
from test_gpu_attn import _bits, _make_layer, _tables
from test_gpu_decode_attn import _chunk, _errors, _ref64

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (32, 8), (28, 4), (14, 2)]
SENT = -1234.0  # fp16 / f32 sentinel; 77 is the int8 one


def _i32(t):
    return t.contiguous().view(torch.int32)


def _raw(t):
    return t.contiguous().view(torch.int8)


def _shuffled_table(g, b, width, dev, spare=1):
    """(int64 [b, width] block ids, num_blocks): a random permutation of b * width + spare blocks; the last `spare` ids of the permutation
    are owned by no row"""
    nb = b * width + spare
    perm = torch.randperm(nb, generator=g, device=dev)
    return perm[:b * width].reshape(b, width), nb, perm[b * width:]


def _to_pool(cache, table, nb, fill):
    """contiguous [b, kvh, W * bs, ...] -> pool [nb, kvh, bs, ...] through table [b, W]; blocks no row owns hold `fill`"""
    b, kvh, cap = cache.shape[:3]
    width = table.shape[1]
    bs = cap // width
    rest = tuple(cache.shape[3:])
    pool = torch.full((nb, kvh, bs) + rest, fill, dtype=cache.dtype, device=cache.device)
    blocks = cache.reshape((b, kvh, width, bs) + rest).transpose(1, 2).reshape((b * width, kvh, bs) + rest)
    pool[table.reshape(-1)] = blocks
    return pool


def _from_pool(pool, table):
    """the inverse: pool [nb, kvh, bs, ...] gathered through table [b, W] -> [b, kvh, W * bs, ...]"""
    b, width = table.shape
    nb, kvh, bs = pool.shape[:3]
    rest = tuple(pool.shape[3:])
    return pool[table.reshape(-1)].reshape((b, width, kvh, bs) + rest).transpose(1, 2).reshape((b, kvh, width * bs) + rest)


def _slots(table, pos, b, bs):
    """slot of every token (token t belongs to row t // s) at position pos[t]"""
    s = pos.numel() // b
    rows = torch.arange(b, device=pos.device).repeat_interleave(s)
    return table[rows, pos // bs] * bs + pos % bs


# ---- the write ops

@pytest.mark.parametrize("bs", [16, 32, 128])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,kvh", SHAPES)
def test_rope_qkv_paged_bit_exact(dev, d, h, kvh, bs):
    from qqq_amd import ops

    cap = 1280
    width = cap // bs
    cos, sin = _tables(dev, 1300, d, seed=d + h)
    g = torch.Generator(device=dev).manual_seed(h * kvh + d + bs)
    for b, s, start in ((1, 7, 0), (3, 1, 1000), (3, 130, 1000), (2, 130, 0)):
        m = b * s
        amp = torch.exp2(torch.randint(-8, 5, (m, 1), generator=g, device=dev).float())
        qkv = (torch.randn((m, (h + 2 * kvh) * d), generator=g, device=dev) * amp).half()
        nq, nk = h * d, kvh * d
        qkv[0, nq:nq + 8] = torch.tensor([30000, -30000, 0, -0.0, 6e-8, -6e-8, 1e-4, 1], dtype=torch.float16)
        qkv[m - 1, nq + nk:nq + nk + d] = 0  # an all-zero v head row
        pos = (start + torch.arange(s, device=dev)).repeat(b)
        table, nb, spare = _shuffled_table(g, b, width, dev, spare=3)
        slots = _slots(table, pos, b, bs)
        views = (qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:])
        for fused in (True, False):
            q, k, v = views if fused else tuple(t.contiguous() for t in views)
            what = (d, h, kvh, bs, b, s, start, fused)
            # fp16: the contiguous cache starts as the sentinel, so equality of the whole gathered pool covers the unwritten slots too
            kc = torch.full((b, kvh, cap, d), SENT, dtype=torch.float16, device=dev)
            vc = kc.clone()
            want_q = ops.rope_qkv(q, k, v, cos, sin, pos, kc, vc).transpose(1, 2).reshape(m, h, d)
            kp = torch.full((nb, kvh, bs, d), SENT, dtype=torch.float16, device=dev)
            vp = kp.clone()
            q_out = ops.rope_qkv_paged(q, k, v, cos, sin, pos, slots, kp, vp)
            assert q_out.shape == (m, h, d) and q_out.is_contiguous()
            assert torch.equal(_bits(q_out), _bits(want_q)), what
            assert torch.equal(_bits(_from_pool(kp, table)), _bits(kc)) and torch.equal(_bits(_from_pool(vp, table)), _bits(vc)), what
            assert bool((kp[spare] == SENT).all()) and bool((vp[spare] == SENT).all()), what
            assert bool((kc[:, :, start:start + s] != SENT).any())
            # int8
            kc8 = torch.full((b, kvh, cap, d), 77, dtype=torch.int8, device=dev)
            ks8 = torch.full((b, kvh, cap), SENT, dtype=torch.float32, device=dev)
            vc8, vs8 = kc8.clone(), ks8.clone()
            want_q8 = ops.rope_qkv_kv8(q, k, v, cos, sin, pos, kc8, vc8, ks8, vs8).transpose(1, 2).reshape(m, h, d)
            kp8 = torch.full((nb, kvh, bs, d), 77, dtype=torch.int8, device=dev)
            ksp = torch.full((nb, kvh, bs), SENT, dtype=torch.float32, device=dev)
            vp8, vsp = kp8.clone(), ksp.clone()
            q_out8 = ops.rope_qkv_paged_kv8(q, k, v, cos, sin, pos, slots, kp8, vp8, ksp, vsp)
            assert torch.equal(_bits(q_out8), _bits(want_q8)) and torch.equal(_bits(q_out8), _bits(want_q)), what
            assert torch.equal(_from_pool(kp8, table), kc8) and torch.equal(_from_pool(vp8, table), vc8), what
            assert torch.equal(_i32(_from_pool(ksp, table)), _i32(ks8)) and torch.equal(_i32(_from_pool(vsp, table)), _i32(vs8)), what
            assert bool((kp8[spare] == 77).all()) and bool((vsp[spare] == SENT).all()), what


@pytest.mark.parametrize("kv8", [False, True])
def test_padding_slots_write_q_only_and_out_of_range_positions_write_nothing(dev, kv8):
    from qqq_amd import ops

    h, kvh, d, bs, nb, m = 8, 2, 128, 16, 6, 12
    cos, sin = _tables(dev, 40, d, seed=3)
    q = torch.randn((m, h * d), device=dev).half()
    k = torch.randn((m, kvh * d), device=dev).half()
    v = torch.randn((m, kvh * d), device=dev).half()
    #                     ok  pad  ok  pos<0  pos=len  slot=n   ok  slot<-1    pos huge  ok  slot huge  ok
    pos = torch.tensor([0, 5, 39, -1, 40, 7, 5, 9, 1 << 40, 12, 3, 39], device=dev)
    slots = torch.tensor([17, -1, 95, 3, 4, nb * bs, 0, -(1 << 40), 8, 33, 1 << 40, 50], device=dev)
    pos_ok = (pos >= 0) & (pos < 40)
    slot_ok = (slots >= 0) & (slots < nb * bs)
    # the reference: the contiguous op with one row of nb * bs slots per token, the token's slot as its position in that row's cache --
    # rope tables indexed by slot would differ, so cos / sin rows are gathered per token instead: token t uses table row t
    cos_t, sin_t = cos[pos.clamp(0, 39)], sin[pos.clamp(0, 39)]
    tpos = torch.arange(m, device=dev)
    if kv8:
        kp = torch.full((nb, kvh, bs, d), 77, dtype=torch.int8, device=dev)
        sp = torch.full((nb, kvh, bs), SENT, dtype=torch.float32, device=dev)
        pools = (kp, kp.clone(), sp, sp.clone())
        q_out = torch.ops.qqq_amd.rope_qkv_paged_kv8(q, k, v, cos, sin, pos, slots, *pools)  # the registered op, eagerly
        ref = (torch.full((1, kvh, m, d), 77, dtype=torch.int8, device=dev), torch.full((1, kvh, m, d), 77, dtype=torch.int8, device=dev),
               torch.full((1, kvh, m), SENT, dtype=torch.float32, device=dev), torch.full((1, kvh, m), SENT, dtype=torch.float32, device=dev))
        want_q = ops.rope_qkv_kv8(q, k, v, cos_t, sin_t, tpos, *ref)
    else:
        kp = torch.full((nb, kvh, bs, d), SENT, dtype=torch.float16, device=dev)
        pools = (kp, kp.clone())
        q_out = torch.ops.qqq_amd.rope_qkv_paged(q, k, v, cos, sin, pos, slots, *pools)
        ref = (torch.full((1, kvh, m, d), SENT, dtype=torch.float16, device=dev), torch.full((1, kvh, m, d), SENT, dtype=torch.float16, device=dev))
        want_q = ops.rope_qkv(q, k, v, cos_t, sin_t, tpos, *ref)
    want_q = want_q.transpose(1, 2).reshape(m, h, d)
    assert torch.equal(_bits(q_out)[pos_ok], _bits(want_q)[pos_ok])  # a padding slot still gets its q_out row
    written = pos_ok & slot_ok
    assert int(written.sum()) == 5
    flat = [p.reshape((nb, kvh, bs) + tuple(p.shape[3:])).transpose(0, 1).reshape((kvh, nb * bs) + tuple(p.shape[3:])) for p in pools]
    mask = torch.zeros(nb * bs, dtype=torch.bool, device=dev)
    mask[slots[written]] = True
    for got, want in zip(flat, ref):
        assert torch.equal(_raw(got[:, slots[written]]), _raw(want[0][:, written]))  # the written rows, bit for bit
        fill = 77 if got.dtype == torch.int8 else SENT
        assert bool((got[:, ~mask] == fill).all())  # nothing else was written


# ---- the decode ops

def _decode_case(dev, g, b, h, kvh, d, cap, bs, kv8):
    """contiguous caches, the pool that holds the same rows through a shuffled table, and one poison block no row owns"""
    k = torch.randn((b, kvh, cap, d), generator=g, device=dev).half()
    v = torch.randn((b, kvh, cap, d), generator=g, device=dev).half()
    table, nb, spare = _shuffled_table(g, b, cap // bs, dev, spare=1)
    if kv8:
        kc, ks = K8.quant_rows_op(k)
        vc, vs = K8.quant_rows_op(v)
        cont = (kc, vc, ks, vs)
        pools = (_to_pool(kc, table, nb, 127), _to_pool(vc, table, nb, 127), _to_pool(ks, table, nb, float("nan")),
                 _to_pool(vs, table, nb, float("nan")))
    else:
        cont = (k, v)
        pools = (_to_pool(k, table, nb, float("nan")), _to_pool(v, table, nb, float("nan")))
    return cont, pools, table, int(spare[0])


def _poisoned(table, pos, bs, poison):
    """int32 table whose entries beyond each row's last block (pos // bs) name the poison block: any read of them shows up as NaN"""
    width = table.shape[1]
    last = (pos.clamp_min(0) // bs)[:, None]
    cols = torch.arange(width, device=table.device)[None]
    return torch.where(cols <= last, table, torch.full_like(table, poison)).to(torch.int32)


def _both(q, cont, pools, table, pos, scale, max_len, kv8):
    from qqq_amd import ops

    q4 = q if q.dim() == 4 else q[:, :, None]  # the contiguous ops take [b, h, 1, d] only
    if kv8:
        want = ops.decode_attention_kv8(q4, *cont, pos, scale, max_len=max_len, return_fp16=True)
        got = ops.decode_attention_paged_kv8(q, *pools, table, pos, scale, max_len=max_len, return_fp16=True)
    else:
        want = ops.decode_attention(q4, *cont, pos, scale, max_len=max_len, return_fp16=True)
        got = ops.decode_attention_paged(q, *pools, table, pos, scale, max_len=max_len, return_fp16=True)
    return got, want


def _assert_same(got, want, what):
    for name, g_, w_ in zip(("xq", "s1", "o_fp16"), got, want):
        assert g_.shape == w_.shape and g_.dtype == w_.dtype, (what, name)
        assert torch.isfinite(g_.float()).all(), (what, name)
        assert torch.equal(_raw(g_), _raw(w_)), (what, name)


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("bs", [16, 32, 128])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,kvh", SHAPES)
def test_decode_attention_paged_bit_exact(dev, d, h, kvh, bs, kv8):
    b, cap = 3, 4224  # 33 blocks of 128
    g = torch.Generator(device=dev).manual_seed(h * 7 + kvh + d + bs)
    cont, pools, table, poison = _decode_case(dev, g, b, h, kvh, d, cap, bs, kv8)
    q = torch.randn((b, h, 1, d), generator=g, device=dev).half()
    c = _chunk(dev, b, kvh, cap)
    for p in [(0, 1, c - 1), (c, c + 1, 4095), (cap - 1, 17, 2 * c + 5)]:
        pos = torch.tensor(p, dtype=torch.int64, device=dev)
        got, want = _both(q, cont, pools, _poisoned(table, pos, bs, poison), pos, d ** -0.5, cap, kv8)
        _assert_same(got, want, (d, h, kvh, bs, kv8, p))
    # q_out as [b, h, d], and a max_len below the table's reach (another split plan)
    pos = torch.tensor((299, 0, 128), dtype=torch.int64, device=dev)
    got, want = _both(q, cont, pools, _poisoned(table, pos, bs, poison), pos, d ** -0.5, 300, kv8)
    _assert_same(got, want, (d, h, kvh, bs, kv8, "max_len 300"))
    got3, _ = _both(q[:, :, 0], cont, pools, _poisoned(table, pos, bs, poison), pos, d ** -0.5, 300, kv8)
    _assert_same(got3, want, (d, h, kvh, bs, kv8, "q_out [b, h, d]"))


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("bs", [16, 128])
def test_rows_that_share_their_first_blocks(dev, bs, kv8):
    h, kvh, d, b, cap = 32, 8, 128, 2, 1024
    g = torch.Generator(device=dev).manual_seed(bs + 17)
    cont, pools, table, poison = _decode_case(dev, g, b, h, kvh, d, cap, bs, kv8)
    q = torch.randn((b, h, 1, d), generator=g, device=dev).half()
    pos = torch.tensor((700, 650), dtype=torch.int64, device=dev)
    shared = 640 // bs  # blocks 0 ... shared-1 hold keys 0 ... 639 of both rows: row 1 names row 0's blocks and keeps its own last ones
    table = table.clone()
    table[1, :shared] = table[0, :shared]
    cont = tuple(t.clone() for t in cont)
    for t in cont:
        t[1, :, :640] = t[0, :, :640]
    got, want = _both(q, cont, pools, _poisoned(table, pos, bs, poison), pos, d ** -0.5, cap, kv8)
    _assert_same(got, want, (bs, kv8))
    assert not torch.equal(_raw(got[2][0]), _raw(got[2][1]))


@pytest.mark.parametrize("kv8", [False, True])
def test_out_of_range_rows_write_nothing_and_a_corrupt_table_stays_inside_the_pool(dev, kv8):
    from qqq_amd import _lib

    h, kvh, d, b, cap, bs, max_len = 32, 8, 128, 5, 512, 32, 300
    g = torch.Generator(device=dev).manual_seed(23)
    cont, pools, table, poison = _decode_case(dev, g, b, h, kvh, d, cap, bs, kv8)
    saved = [t.clone() for t in pools]
    q = torch.randn((b, h, 1, d), generator=g, device=dev).half()
    pos = torch.tensor([-1, 299, 300, cap, 100], dtype=torch.int64, device=dev)  # rows 1 and 4 are in [0, max_len)
    tab = _poisoned(table, pos, bs, poison)
    tab[0], tab[2], tab[3] = -7, 1 << 30, -(1 << 31)  # rows that are never read
    tab[4, 1] = 1 << 30  # a corrupt entry that IS read: clamped into the pool, the row's result is unspecified but finite garbage at worst
    o = torch.full((b, h * d), SENT, dtype=torch.float16, device=dev)
    xq = torch.full((b, h * d), 77, dtype=torch.int8, device=dev)
    s1 = torch.full((b, 1), SENT, dtype=torch.float32, device=dev)
    L = _lib.lib()
    nbytes = L.qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    tail = (tab.data_ptr(), tab.shape[1], pos.data_ptr(), d ** -0.5, o.data_ptr(), xq.data_ptr(), s1.data_ptr(), ws.data_ptr(), nbytes, b, h,
            kvh, d, pools[0].shape[0], bs, max_len, 0, torch.cuda.current_stream().cuda_stream)
    fn = L.qqq_decode_attn_paged_kv8 if kv8 else L.qqq_decode_attn_paged
    err = fn(q.data_ptr(), *(t.data_ptr() for t in pools), *tail)
    torch.cuda.synchronize()
    assert err == 0, _lib.last_error()
    for bi in (0, 2, 3):
        assert bool((o[bi] == SENT).all()) and bool((xq[bi] == 77).all()) and float(s1[bi]) == SENT, bi
    for t, t0 in zip(pools, saved):
        assert torch.equal(_raw(t), _raw(t0))  # the pools are only read
    assert bool((o[4] != SENT).any())
    got, want = _both(q[1:2], tuple(t[1:2] for t in cont), pools, tab[1:2], pos[1:2], d ** -0.5, max_len, kv8)
    _assert_same(got, want, "row 1 alone")
    # b = 1 has another split plan than b = 5: the row inside the batch is compared with the contiguous op at b = 5
    _, want5 = _both(q, cont, pools, tab, pos.clamp(0, max_len - 1), d ** -0.5, max_len, kv8)
    assert torch.equal(_raw(o[1]), _raw(want5[2][1])) and torch.equal(xq[1], want5[0][1]) and torch.equal(_i32(s1[1]), _i32(want5[1][1]))


@pytest.mark.parametrize("kv8", [False, True])
def test_decode_attention_paged_against_float64(dev, kv8):
    """The absolute anchor of the bit-exact chain: relative L2 per (row, head) <= 1e-3 and max error <= 2^-9 max|v|, the bounds of
    tests/test_gpu_decode_attn.py and tests/test_gpu_kv8.py."""
    h, kvh, d, b, cap, bs = 32, 8, 128, 3, 4224, 16
    g = torch.Generator(device=dev).manual_seed(31)
    cont, pools, table, poison = _decode_case(dev, g, b, h, kvh, d, cap, bs, kv8)
    q = torch.randn((b, h, 1, d), generator=g, device=dev).half()
    pos = torch.tensor((cap - 1, 17, 2077), dtype=torch.int64, device=dev)
    got, _ = _both(q, cont, pools, _poisoned(table, pos, bs, poison), pos, d ** -0.5, cap, kv8)
    if kv8:
        k64, v64 = K8.dequant64(_from_pool(pools[0], table), _from_pool(pools[2], table)), K8.dequant64(_from_pool(pools[1], table),
                                                                                                      _from_pool(pools[3], table))
        ref = K8.attention64(q, k64, v64, pos, d ** -0.5)
    else:
        k64, v64 = _from_pool(pools[0], table), _from_pool(pools[1], table)
        ref = _ref64(q, k64, v64, pos, d ** -0.5)
    rel, mx = _errors(got[2], ref, v64, pos)
    print(f"decode_attention_paged{'_kv8' if kv8 else ''} vs float64: rel L2 {rel:.2e}, max|err|/max|v| {mx:.2e} (2^-9 = {2 ** -9:.2e})")
    assert rel <= 1e-3 and mx <= 2 ** -9, (rel, mx)


# ---- hipGraph and torch.compile

@pytest.mark.parametrize("kv8", [False, True])
def test_hipgraph_replays_with_pos_slots_and_table_updated_in_place(dev, kv8):
    from qqq_amd import ops

    h, kvh, d, b, bs, width = 32, 8, 128, 2, 16, 8
    nb, cap = 20, width * bs
    g = torch.Generator(device=dev).manual_seed(41)
    cos, sin = _tables(dev, cap, d, seed=5)
    perm = torch.randperm(nb, generator=g, device=dev).tolist()
    owned = [[perm.pop()], [perm.pop(), perm.pop()]]  # sequence 0 holds 14 keys (one block), sequence 1 holds 30 (two)
    lengths = [14, 30]

    def pools_like():
        if kv8:
            return (torch.zeros((nb, kvh, bs, d), dtype=torch.int8, device=dev), torch.zeros((nb, kvh, bs, d), dtype=torch.int8, device=dev),
                    torch.zeros((nb, kvh, bs), device=dev), torch.zeros((nb, kvh, bs), device=dev))
        return (torch.zeros((nb, kvh, bs, d), dtype=torch.float16, device=dev), torch.zeros((nb, kvh, bs, d), dtype=torch.float16, device=dev))

    write = ops.rope_qkv_paged_kv8 if kv8 else ops.rope_qkv_paged
    decode = ops.decode_attention_paged_kv8 if kv8 else ops.decode_attention_paged
    nq, nk = h * d, kvh * d

    def step(qkv, pos, slots, table, pools):
        q_out = write(qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:], cos, sin, pos, slots, *pools)
        return (q_out,) + tuple(decode(q_out, *pools, table, pos, d ** -0.5, max_len=cap, return_fp16=True))

    pg = pools_like()
    # the history, written eagerly
    hist_pos = torch.tensor([p for n in lengths for p in range(n)], device=dev)
    hist_slots = torch.tensor([owned[i][p // bs] * bs + p % bs for i, n in enumerate(lengths) for p in range(n)], device=dev)
    hist = torch.randn((hist_pos.numel(), (h + 2 * kvh) * d), generator=g, device=dev).half()
    write(hist[:, :nq], hist[:, nq:nq + nk], hist[:, nq + nk:], cos, sin, hist_pos, hist_slots, *pg)
    pe = tuple(t.clone() for t in pg)

    qkv = torch.randn((b, (h + 2 * kvh) * d), generator=g, device=dev).half()
    pos = torch.zeros(b, dtype=torch.int64, device=dev)
    slots = torch.full((b,), -1, dtype=torch.int64, device=dev)  # the warm-up and the capture write no cache row
    table = torch.zeros((b, width), dtype=torch.int32, device=dev)
    for i in range(b):
        table[i, :len(owned[i])] = torch.tensor(owned[i], dtype=torch.int32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(qkv, pos, slots, table, pg)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = step(qkv, pos, slots, table, pg)
    torch.cuda.current_stream().wait_stream(side)
    for t_, e_ in zip(pg, pe):
        assert torch.equal(_raw(t_), _raw(e_))  # padding slots: warm-up and capture left the pools alone
    for it in range(5):  # positions 14 ... 18 and 30 ... 34: both sequences cross a block boundary (16, 32)
        for i in range(b):
            if lengths[i] % bs == 0:
                owned[i].append(perm.pop())
                table[i, len(owned[i]) - 1] = owned[i][-1]
        pos.copy_(torch.tensor(lengths, device=dev))
        slots.copy_(torch.tensor([owned[i][lengths[i] // bs] * bs + lengths[i] % bs for i in range(b)], device=dev))
        qkv.copy_(torch.randn(qkv.shape, generator=g, device=dev).half())
        graph.replay()
        torch.cuda.synchronize()
        want = step(qkv, pos, slots, table, pe)
        for g_, w_ in zip(out, want):
            assert torch.equal(_raw(g_), _raw(w_)), (kv8, it)
        for t_, e_ in zip(pg, pe):
            assert torch.equal(_raw(t_), _raw(e_)), (kv8, it)
        lengths = [n + 1 for n in lengths]
    assert [len(o) for o in owned] == [2, 3]


def test_paged_ops_trace_under_torch_compile(dev):
    from qqq_amd import ops

    h, kvh, d, b, bs, width = 28, 4, 128, 2, 32, 8
    g = torch.Generator(device=dev).manual_seed(9)
    cos, sin = _tables(dev, width * bs, d, seed=11)
    table64, nb, _ = _shuffled_table(g, b, width, dev)
    table = table64.to(torch.int32)
    pos = torch.tensor([200, 31], dtype=torch.int64, device=dev)
    slots = _slots(table64, pos, b, bs)
    qkv = torch.randn((b, (h + 2 * kvh) * d), generator=g, device=dev).half()
    nq, nk = h * d, kvh * d
    k16 = torch.randn((nb, kvh, bs, d), generator=g, device=dev).half()
    v16 = torch.randn((nb, kvh, bs, d), generator=g, device=dev).half()
    k8, ks = K8.quant_rows_op(k16)
    v8, vs = K8.quant_rows_op(v16)

    def f(qkv, k16, v16, k8, v8, ks, vs, pos, slots, table):
        q1 = ops.rope_qkv_paged(qkv[:, :nq] * 1, qkv[:, nq:nq + nk], qkv[:, nq + nk:], cos, sin, pos, slots, k16, v16)
        xq, s1, o = ops.decode_attention_paged(q1, k16, v16, table, pos, d ** -0.5, return_fp16=True)
        q2 = ops.rope_qkv_paged_kv8(qkv[:, :nq] * 1, qkv[:, nq:nq + nk], qkv[:, nq + nk:], cos, sin, pos, slots, k8, v8, ks, vs)
        xq8, s18, o8 = ops.decode_attention_paged_kv8(q2, k8, v8, ks, vs, table, pos, d ** -0.5, return_fp16=True)
        return q1, xq, s1 * 2, o, q2, xq8, s18 * 2, o8

    c1 = [t.clone() for t in (k16, v16, k8, v8, ks, vs)]
    c2 = [t.clone() for t in (k16, v16, k8, v8, ks, vs)]
    eager = f(qkv, *c1, pos, slots, table)
    comp = torch.compile(f, fullgraph=True)(qkv, *c2, pos, slots, table)
    for e, c in zip(eager, comp):
        assert torch.equal(_raw(e), _raw(c))
    for a, b_, orig in zip(c1, c2, (k16, v16, k8, v8, ks, vs)):
        assert torch.equal(_raw(a), _raw(b_)) and not torch.equal(_raw(a), _raw(orig))


# ---- the decoder layer over a PagedKVCache

def _rel(got, want):
    return float((got.float() - want.float()).norm() / want.float().norm())


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_layer_with_uniform_lengths_equals_the_contiguous_cache(dev, dtype):
    from qqq_amd import KVCache, PagedKVCache

    hidden, heads, kvh, inter = 1024, 8, 2, 2048
    layer = _make_layer(dev, hidden, heads, kvh, inter, 128, False, seed=61).eval()
    if dtype == torch.float16:
        layer.fuse_decode()  # the contiguous fp16 cache takes its decode kernel only when asked; the paged and the int8 cache always do
    b, pre, steps, d, bs = 3, 37, 6, hidden // heads, 16
    xs = torch.randn((b, pre + steps, hidden), device=dev).half()
    cont = KVCache(1, b, kvh, d, 64, dev, dtype=dtype)
    paged = PagedKVCache(1, 3 * b + 2, kvh, d, bs, dev, dtype=dtype)
    for i in range(b):
        paged.add(i)
    want = layer(xs[:, :pre], cont, 0)
    st = paged.step(range(b), [pre] * b)
    assert not st.decode and st.max_len == pre
    got = layer(xs[:, :pre].reshape(b * pre, hidden), paged, st).reshape(b, pre, hidden)
    rel = _rel(got, want)
    print(f"paged layer ({dtype}), packed prefill of {b} x {pre}: relative L2 vs the contiguous cache {rel:.2e}")
    assert torch.isfinite(got).all() and rel <= 1e-2, rel
    for t in range(pre, pre + steps):
        want = layer(xs[:, t:t + 1], cont, t)
        st = paged.step(range(b), [1] * b)
        assert st.decode and st.max_len == t + 1
        got = layer(xs[:, t], paged, st)
        assert torch.equal(_bits(got), _bits(want[:, 0])), (dtype, t)  # decode steps: bit for bit
    for i in range(b):  # ... and the pools hold the contiguous cache's rows
        n = pre + steps
        kg, vg = paged.gather(0, i)
        if dtype == torch.int8:
            kc, vc = cont.dequant(0, n)
        else:
            kc, vc = cont.k[0][:, :, :n], cont.v[0][:, :, :n]
        assert torch.equal(_bits(kg[0]), _bits(kc[i])) and torch.equal(_bits(vg[0]), _bits(vc[i]))


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_layer_with_ragged_lengths_and_a_recycled_sequence(dev, dtype):
    """Sequences of 5, 70 and 133 tokens in one packed prefill, three decode steps, the shortest freed and a 20-token sequence admitted into
    its blocks, three more decode steps: every sequence's outputs against the same layer run alone on KVCache(batch=1).  The split plan
    depends on b, so bits may differ: relative L2 <= 1e-2, the bound tests/test_gpu_decode_attn.py uses between decode paths."""
    from qqq_amd import KVCache, PagedKVCache

    hidden, heads, kvh, inter = 1024, 8, 2, 2048
    layer = _make_layer(dev, hidden, heads, kvh, inter, 128, False, seed=63).eval()
    if dtype == torch.float16:
        layer.fuse_decode()
    d, bs = hidden // heads, 16
    pre = {"a": 5, "b": 70, "c": 133, "n": 20}
    total = {"a": 5 + 3, "b": 70 + 6, "c": 133 + 6, "n": 20 + 3}
    g = torch.Generator(device=dev).manual_seed(7)
    xs = {sid: torch.randn((n, hidden), generator=g, device=dev).half() for sid, n in total.items()}
    got = {sid: [] for sid in total}
    paged = PagedKVCache(1, 1 + 5 + 9 + 1, kvh, d, bs, dev, dtype=dtype)  # a: 1 block, b: 5, c: 9, and one to spare
    done = {sid: 0 for sid in total}

    def run(sids, counts):
        st = paged.step(sids, counts)
        x = torch.cat([xs[s][done[s]:done[s] + c] for s, c in zip(sids, counts)])
        out = layer(x, paged, st)
        assert torch.isfinite(out).all()
        t = 0
        for s, c in zip(sids, counts):
            got[s].append(out[t:t + c])
            done[s] += c
            t += c
        return st

    for sid in ("a", "b", "c"):
        paged.add(sid)
    st = run(["a", "b", "c"], [5, 70, 133])
    assert not st.decode and st.max_len == 133 and paged.free_blocks == 1
    for _ in range(3):
        assert run(["a", "b", "c"], [1, 1, 1]).decode
    freed = paged.blocks("a")
    paged.free("a")
    paged.add("n")
    st = run(["n"], [20])  # admitted in a step of its own: two blocks, the freed one first
    assert not st.decode and set(freed) <= set(paged.blocks("n")) and paged.blocks("n")[0] == freed[-1]
    for _ in range(3):
        assert run(["b", "c", "n"], [1, 1, 1]).decode
    assert done == total
    worst = 0.0
    for sid, n in total.items():
        alone = KVCache(1, 1, kvh, d, 160, dev, dtype=dtype)
        want = [layer(xs[sid][None, :pre[sid]], alone, 0)[0]]
        want += [layer(xs[sid][None, t:t + 1], alone, t)[0] for t in range(pre[sid], n)]
        assert len(want) == len(got[sid])
        for i, (g_, w_) in enumerate(zip(got[sid], want)):
            rel = _rel(g_, w_)
            worst = max(worst, rel)
            assert rel <= 1e-2, (dtype, sid, i, rel)
        kg, vg = paged.gather(0, sid) if sid != "a" else (None, None)
        if sid != "a":  # the cache rows do not depend on the batch: bit for bit the rows of the run alone
            kc, vc = alone.dequant(0, n) if dtype == torch.int8 else (alone.k[0][:, :, :n], alone.v[0][:, :, :n])
            assert torch.equal(_bits(kg), _bits(kc)) and torch.equal(_bits(vg), _bits(vc)), sid
    print(f"paged layer ({dtype}), ragged and recycled: worst relative L2 vs each sequence alone {worst:.2e}")
