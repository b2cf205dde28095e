"""The shared-prefix decode attention on the GPU (include/qqq_amd_shared.h): o_fp16, xq and s1 of every row bit for bit those of
decode_attention_paged(_kv8) called on the same tensors, over both pools, head shapes, packs of one, two and four query tiles, families of
every size around the pack, shared lengths around the chunk, retired rows anywhere in a pack, senseless descriptors, and hipGraph replay
with families, shared lengths and positions changed in place.

b <= 24, kvh <= 4 and max_len = 1024 throughout, so the split plan is eight chunks of 128 keys (b * kvh <= 96 leaves at least eight
planned splits on any device of 192 compute units or more; with a larger kvh the plan has fewer and longer chunks; asserted through the
plan entry point): a family with shared >= 128 has shared // 128 jointly taken chunks.  The library entry points are called directly
where the workspace and the outputs have to be the test's own: the workspace is filled with NaN before each call, the outputs with a
sentinel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_LEN, CHUNK = 1024, 128
SENT = -1234.0


def _raw(t):
    return t.contiguous().view(torch.int8)


def _pools(dev, g, nb, kvh, bs, d, kv8):
    """a pool whose every block holds finite random rows: any table is a valid one"""
    if kv8:
        k = torch.randint(-127, 128, (nb, kvh, bs, d), generator=g, device=dev, dtype=torch.int8)
        v = torch.randint(-127, 128, (nb, kvh, bs, d), generator=g, device=dev, dtype=torch.int8)
        ks = torch.rand((nb, kvh, bs), generator=g, device=dev) * 0.02 + 0.001
        vs = torch.rand((nb, kvh, bs), generator=g, device=dev) * 0.02 + 0.001
        return (k, v, ks, vs)
    return (torch.randn((nb, kvh, bs, d), generator=g, device=dev).half(), torch.randn((nb, kvh, bs, d), generator=g, device=dev).half())


def _case(dev, g, families, bs, kvh, d, kv8, whole_blocks=True):
    """families: [(size, shared, [pos per member])].  Every row gets blocks of its own; the rows of a family then take the first row's
    ids for their first shared // bs blocks.  shared is a multiple of bs unless whole_blocks is False: then the block that holds the end
    of the prefix stays a block of each sibling's own, and its first shared % bs rows are copies of the first row's (what copy-on-write
    of a partial block leaves).  -> pools, table, pos, family, shared (device tensors)"""
    b = sum(f[0] for f in families)
    width = MAX_LEN // bs
    nb = b * width + 3
    perm = torch.randperm(nb, generator=g, device=dev)
    table = perm[:b * width].reshape(b, width).clone()
    fam, sh, pos, r, copies = [], [], [], 0, []
    for size, shared, ps in families:
        assert (shared % bs == 0 or not whole_blocks) and len(ps) == size
        for j in range(size):
            table[r + j, :shared // bs] = table[r, :shared // bs]
            if shared % bs and j:
                copies.append((int(table[r + j, shared // bs]), int(table[r, shared // bs]), shared % bs))
            fam.append(r)
            sh.append(shared if size > 1 else 0)
        pos += ps
        r += size
    i64 = dict(dtype=torch.int64, device=dev)
    pools = _pools(dev, g, nb, kvh, bs, d, kv8)
    for dst, src, n in copies:
        for t in pools:
            t[dst, :, :n] = t[src, :, :n]
    return (pools, table.to(torch.int32), torch.tensor(pos, **i64),
            torch.tensor(fam, dtype=torch.int32, device=dev), torch.tensor(sh, **i64))


def _plain(q, pools, table, pos, scale, kv8):
    from qqq_amd import ops

    op = ops.decode_attention_paged_kv8 if kv8 else ops.decode_attention_paged
    return op(q, *pools, table, pos, scale, max_len=MAX_LEN, return_fp16=True)


def _shared(q, pools, table, pos, family, shared, pack, scale, kv8):
    """the library call with a workspace of NaN and outputs of sentinels -> (xq, s1, o_fp16)"""
    from qqq_amd import _lib, ops

    L = _lib.lib()
    b, h, d = q.shape
    nb, kvh, bs = pools[0].shape[:3]
    dev = q.device
    xq = torch.full((b, h * d), 77, dtype=torch.int8, device=dev)
    s1 = torch.full((b, 1), SENT, dtype=torch.float32, device=dev)
    o16 = torch.full((b, h * d), SENT, dtype=torch.float16, device=dev)
    nbytes = L.qqq_decode_attn_workspace_bytes(b, h, kvh, d, MAX_LEN)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev)
    P = ops._ptr
    tail = (P(table), table.shape[1], P(pos), P(family), P(shared), pack, float(scale), P(o16), P(xq), P(s1), P(ws), nbytes, b, h, kvh, d, nb,
            bs, MAX_LEN, dev.index or 0, ops._stream_for(q))
    fn = L.qqq_decode_attn_paged_shared_kv8 if kv8 else L.qqq_decode_attn_paged_shared
    err = fn(*(P(t) for t in (q,) + tuple(pools)), *tail)
    assert err == 0, _lib.last_error()
    torch.cuda.synchronize()
    return xq, s1, o16


def _joint_chunks(b, h, kvh, pack, shared):
    from qqq_amd import ops

    splits, chunk = ops.decode_attention_shared_plan(b, h, kvh, MAX_LEN, pack)
    assert chunk == CHUNK and splits == MAX_LEN // CHUNK  # the plan of the docstring
    return shared // chunk


def _assert_rows_equal(got, want, pos, what, untouched=()):
    for r in range(pos.numel()):
        live = 0 <= int(pos[r]) < MAX_LEN
        assert live != (r in untouched), (what, r)
        for name, g_, w_ in zip(("xq", "s1", "o_fp16"), got, want):
            if live:
                assert torch.isfinite(g_[r].float()).all(), (what, name, r)
                assert torch.equal(_raw(g_[r]), _raw(w_[r])), (what, name, r)
            else:  # a retired row writes nothing
                assert bool((g_[r] == (77 if name == "xq" else SENT)).all()), (what, name, r)


def _positions(g, size, shared, chunk=CHUNK):
    """a member whose last key is the first one behind the prefix (pos = shared), one that has just been forked (pos = shared - 1), one in
    the chunk right behind the prefix, one several chunks later, the rest anywhere behind the prefix"""
    fixed = [shared, max(shared - 1, 0), shared + 5, min(shared + 3 * chunk + 17, MAX_LEN - 1), MAX_LEN - 1]
    rest = [int(torch.randint(shared, MAX_LEN, (1,), generator=g)) for _ in range(max(0, size - len(fixed)))]
    return (fixed + rest)[:size]


# (h, kvh, pack): h / kvh of 8, 4 and 1; G * pack of one, two and four 16-row tiles
COMBOS = [(8, 1, 2), (8, 1, 4), (8, 1, 8), (8, 2, 4), (8, 2, 8), (8, 2, 16), (4, 4, 3), (4, 4, 20)]


def _layouts(pack):
    """family sizes 1, 2, exactly pack and pack + 1 (two packs), two or more families and lone rows in one call, b <= 24; shared of 0, of
    64 (below one chunk: nothing joint), of exactly 128 and of 384"""
    if 2 * pack + 5 <= 24:
        return [[(pack + 1, 384), (1, 0), (2, 128), (pack, 64), (1, 0)], [(pack, 384), (2, 0), (pack + 1, 128)]]
    return [[(pack + 1, 384), (1, 0), (2, 128)], [(pack, 384), (1, 0), (2, 64)], [(pack, 128), (3, 0)]]


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("bs", [16, 256])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,kvh,pack", COMBOS)
def test_every_row_equals_the_plain_op(dev, h, kvh, pack, d, bs, kv8):
    g = torch.Generator(device=dev).manual_seed(h * 7 + kvh * 3 + pack + d + bs)
    cg = torch.Generator().manual_seed(pack)
    for layout in _layouts(pack):
        if bs == 256:  # whole blocks are shared: two and one of them, and none
            layout = [(n, {384: 512, 128: 256, 64: 0, 0: 0}[s]) for n, s in layout]
        fams = [(n, s, _positions(cg, n, s)) for n, s in layout]
        b = sum(n for n, _ in layout)
        assert b <= 24
        for n, s in layout:
            if n > 1 and s >= CHUNK:
                assert _joint_chunks(b, h, kvh, pack, s) >= 1  # the case does contain jointly taken chunks
        pools, table, pos, family, shared = _case(dev, g, fams, bs, kvh, d, kv8)
        q = torch.randn((b, h, d), generator=g, device=dev).half()
        want = _plain(q, pools, table, pos, d ** -0.5, kv8)
        got = _shared(q, pools, table, pos, family, shared, pack, d ** -0.5, kv8)
        _assert_rows_equal(got, want, pos, (layout, h, kvh, pack, d, bs, kv8))


@pytest.mark.parametrize("kv8", [False, True])
def test_pack_one_is_the_plain_op(dev, kv8):
    g = torch.Generator(device=dev).manual_seed(5)
    fams = [(3, 384, [384, 500, 1023]), (1, 0, [77])]
    pools, table, pos, family, shared = _case(dev, g, fams, 16, 2, 128, kv8)
    q = torch.randn((4, 8, 128), generator=g, device=dev).half()
    _assert_rows_equal(_shared(q, pools, table, pos, family, shared, 1, 0.09, kv8), _plain(q, pools, table, pos, 0.09, kv8), pos, "pack 1")


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("retired", [[2], [0], [4], [0, 1, 2, 3, 4], [1, 3, 6]])
def test_retired_rows_write_nothing_and_disturb_nobody(dev, retired, kv8):
    """a family of five in packs of four (rows 0 ... 3 and 4) and one of two: a retired sibling in the middle of a pack, a retired first
    row of a pack and of a family (its table row names other valid blocks), a retired one-row pack, a whole family retired, and rows
    retired past max_len as well as below 0"""
    g = torch.Generator(device=dev).manual_seed(11 + len(retired) + retired[0])
    fams = [(5, 384, [384, 390, 700, 1023, 511]), (2, 256, [256, 300])]
    assert _joint_chunks(7, 8, 2, 4, 384) == 3
    pools, table, pos, family, shared = _case(dev, g, fams, 16, 2, 128, kv8)
    q = torch.randn((7, 8, 128), generator=g, device=dev).half()
    nb = pools[0].shape[0]
    for i, r in enumerate(retired):
        pos[r] = -1 if i % 2 == 0 else MAX_LEN + 3
        table[r] = torch.randint(0, nb, (table.shape[1],), generator=g, device=dev).to(torch.int32)  # anything, and valid ids
    want = _plain(q, pools, table, pos, 0.09, kv8)
    got = _shared(q, pools, table, pos, family, shared, 4, 0.09, kv8)
    _assert_rows_equal(got, want, pos, ("retired", retired, kv8), untouched=retired)


@pytest.mark.parametrize("kv8", [False, True])
def test_senseless_descriptors_make_rows_compute_alone(dev, kv8):
    g = torch.Generator(device=dev).manual_seed(23)
    fams = [(4, 384, [384, 400, 200, 1023]), (3, 128, [128, 129, 600])]
    pools, table, pos, family, shared = _case(dev, g, fams, 16, 2, 64, kv8)
    # row 2 of the first family stands at key 200: what it shares is clamped to its own 201 keys, one chunk
    q = torch.randn((7, 8, 64), generator=g, device=dev).half()
    want = _plain(q, pools, table, pos, 0.125, kv8)
    big = torch.iinfo(torch.int64).max
    for fam, sh in (([0, 0, 0, 0, 4, 4, 4], [384, 384, 384, 384, 128, 128, 128]),   # the sane descriptors, but for row 2
                    ([3, 0, -1, 99, 5, 4, 1 << 30], [384] * 7),                       # forward, negative and far names
                    ([0, 0, 1, 2, 4, 5, 5], [384, 384, 384, 384, 128, 128, 128]),   # names of rows that are no roots
                    ([0, 0, 0, 0, 4, 4, 4], [big, big, -5, -big, 1 << 40, 0, 128])):   # shared beyond pos + 1 and below 0
        family = torch.tensor(fam, dtype=torch.int32, device=dev)
        shared = torch.tensor(sh, dtype=torch.int64, device=dev)
        got = _shared(q, pools, table, pos, family, shared, 4, 0.125, kv8)
        _assert_rows_equal(got, want, pos, ("descriptors", fam, sh, kv8))


@pytest.mark.parametrize("kv8", [False, True])
def test_hipgraph_replays_with_families_shared_and_pos_changed_in_place(dev, kv8):
    from qqq_amd import ops

    g = torch.Generator(device=dev).manual_seed(31)
    h, kvh, d, bs, pack, b = 8, 2, 128, 16, 4, 8
    fams = [(4, 384, [384, 385, 600, 1000]), (1, 0, [50]), (3, 128, [128, 140, 900])]
    pools, table, pos, family, shared = _case(dev, g, fams, bs, kvh, d, kv8)
    q = torch.randn((b, h, d), generator=g, device=dev).half()
    op = ops.decode_attention_paged_shared_kv8 if kv8 else ops.decode_attention_paged_shared
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        op(q, *pools, table, pos, family, shared, pack, 0.09, max_len=MAX_LEN, return_fp16=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = op(q, *pools, table, pos, family, shared, pack, 0.09, max_len=MAX_LEN, return_fp16=True)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    _assert_rows_equal(out, _plain(q, pools, table, pos, 0.09, kv8), pos, "captured")
    # other families (2 + 5 + 1), other shared lengths, other positions, a retired row, other queries: all in place
    fams2 = [(2, 640, [640, 1023]), (5, 256, [256, 255, -1, 300, 777]), (1, 0, [3])]
    _, table2, pos2, family2, shared2 = _case(dev, g, fams2, bs, kvh, d, kv8)
    table.copy_(table2.clamp_max(pools[0].shape[0] - 1))
    for dst, src in ((pos, pos2), (family, family2), (shared, shared2)):
        dst.copy_(src)
    q.copy_(torch.randn((b, h, d), generator=g, device=dev).half())
    graph.replay()
    torch.cuda.synchronize()
    want = _plain(q, pools, table, pos, 0.09, kv8)
    for r in range(b):
        if int(pos[r]) < 0:
            continue
        for name, g_, w_ in zip(("xq", "s1", "o_fp16"), out, want):
            assert torch.equal(_raw(g_[r]), _raw(w_[r])), ("replayed", name, r)


def test_the_ops_refuse_what_the_library_refuses(dev):
    from qqq_amd import ops

    g = torch.Generator(device=dev).manual_seed(41)
    pools, table, pos, family, shared = _case(dev, g, [(2, 128, [128, 200])], 16, 2, 64, False)
    q = torch.randn((2, 8, 64), generator=g, device=dev).half()
    with pytest.raises(RuntimeError, match="pack"):
        ops.decode_attention_paged_shared(q, *pools, table, pos, family, shared, 0, 0.1, max_len=MAX_LEN)
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.decode_attention_paged_shared(q, *pools, table, pos, family, shared, 17, 0.1, max_len=MAX_LEN)  # 4 * 17 > 64 query rows
    with pytest.raises(RuntimeError, match="family must be int32"):
        ops.decode_attention_paged_shared(q, *pools, table, pos, family.long(), shared, 2, 0.1, max_len=MAX_LEN)
    with pytest.raises(RuntimeError, match="entries"):
        ops.decode_attention_paged_shared(q, *pools, table, pos, family[:1], shared, 2, 0.1, max_len=MAX_LEN)
