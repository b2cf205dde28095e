"""The two kernels that place several query rows per KV head into the 16-row MFMA tiles of the decode split kernel, at every documented
head layout and under other split plans than their own files use: qqq_verify_attn_paged(_kv8) (query row tok * G + g,
include/qqq_amd_verify.h) and qqq_decode_attn_paged_shared(_kv8) (query row slot * G + g with a live-slot set per job,
include/qqq_amd_shared.h).  G = h / kvh from 1 to 8, with the G that do not divide 16 (a token's or a sibling's rows then lie in two tiles),
h*d on both sides of 4096 and 8192 (one, two and four 16-byte vectors per thread of the combine kernels), block sizes 16, 128 and 256,
plans with chunks of 256 and 384 keys, and a max_len that is no multiple of the chunk.

Both headers promise the outputs of decode_attention_paged(_kv8) bit for bit, and tests/test_gpu_head_layouts.py holds that op to float64
at every layout: the reference of every case here is that op on the same tensors, and one float64 check per kernel and pool dtype (the
bounds of tests/test_gpu_decode_attn.py) anchors the chain.  The library entry points are called directly: the workspace is NaN before
every call and the outputs hold a sentinel, so a partial the combine reads but nobody wrote is a NaN in the output.

The case tables are built by module-level functions that need no GPU.  tests/test_shared_ref_cpu.py runs them with the plan of a device
of 256 compute units through the model of tests/shared_ref.py and asserts that every case does put through the kernel what it is there
for; the tests here repeat those assertions with the plan of the device they run on."""
import pytest
import torch

import kv8_ref as K8
import shared_ref as REF
import test_gpu_shared_attn as SH
from test_gpu_decode_attn import _chunk, _errors, _ref64
from test_gpu_head_layouts import _assert_quant_exact
from test_gpu_paged import SENT, _decode_case, _from_pool
from test_gpu_verify import _assert_tokens_equal_decode, _poisoned_chunk

pytestmark = pytest.mark.gpu

COMBINE_NT = 512  # threads of a combine workgroup, one 16-byte vector of eight outputs each: h*d <= 4096 is one vector per thread


def tiles_of(rows):
    """16-row tiles of the instantiation a call with this many query rows per KV head runs"""
    return 1 if rows <= 16 else 2 if rows <= 32 else 4


def combine_vectors(h, d):
    n = h * d // 8
    return 1 if n <= COMBINE_NT else 2 if n <= 2 * COMBINE_NT else 4


def straddlers(G, n):
    """the tokens (slots) below n whose G query rows lie in two tiles"""
    return [s for s in range(n) if (s * G) // 16 != (s * G + G - 1) // 16]


# ---- the verify chunk

V_B, V_MAX_LEN = 4, 640
#               h, kvh,   d,  t    G  rows  tiles  vectors  first token in two tiles
VERIFY_CASES = [(16, 8, 64, 16,    2, 32, 2, 1, None),   # G = 2; two full tiles
                (24, 8, 128, 11,   3, 33, 4, 1, 5),      # one row in the third tile, the fourth all padding
                (33, 11, 128, 5,   3, 15, 1, 2, None),   # one head past 4096
                (40, 8, 128, 12,   5, 60, 4, 2, 3),      # G = 5
                (65, 13, 128, 3,   5, 15, 1, 4, None),   # one head past 8192
                (96, 16, 64, 10,   6, 60, 4, 2, 2),      # G = 6
                (96, 16, 128, 3,   6, 18, 2, 4, 2),
                (28, 4, 128, 9,    7, 63, 4, 1, 2),
                (64, 8, 128, 8,    8, 64, 4, 2, None),   # four full tiles; the upper end of two vectors
                (128, 16, 128, 2,  8, 16, 1, 4, None),   # the maximum
                (128, 16, 128, 8,  8, 64, 4, 4, None),
                (40, 40, 128, 16,  1, 16, 1, 2, None),
                (128, 64, 64, 16,  2, 32, 2, 2, None)]   # b * kvh = 256: a plan of longer chunks where the device has 256 compute units
VERIFY_ONE_PER_G = [(16, 8, 64, 16), (24, 8, 128, 11), (40, 8, 128, 12), (96, 16, 64, 10), (64, 8, 128, 8)]  # G = 2, 3, 5, 6, 8


def check_verify_case(h, kvh, d, t, G, rows, tiles, vectors, straddler):
    """the arithmetic the table claims, and the limits of the entry points"""
    assert h % kvh == 0 and h // kvh == G and 1 <= G <= 8 and d in (64, 128) and h * d <= 16384
    assert 1 <= t <= 16 and G * t == rows <= 64 and tiles_of(rows) == tiles and combine_vectors(h, d) == vectors
    s = straddlers(G, t)
    assert (s[0] if s else None) == straddler, s
    assert (16 % G != 0) == (G in (3, 5, 6, 7))
    if 16 % G != 0 and rows > 16:
        assert s  # where G does not divide 16 and there is a second tile, some token's rows lie in two tiles


def _verify_lib(q, pools, table, start, t, scale, max_len, kv8):
    """the library call with a workspace of NaN and outputs of sentinels -> (xq, s1, o_fp16)"""
    from qqq_amd import _lib, ops

    L = _lib.lib()
    rows, h, d = q.shape
    b = start.numel()
    assert rows == b * t
    nb, kvh, bs = pools[0].shape[:3]
    dev = q.device
    xq = torch.full((rows, h * d), 77, dtype=torch.int8, device=dev)
    s1 = torch.full((rows, 1), SENT, dtype=torch.float32, device=dev)
    o16 = torch.full((rows, h * d), SENT, dtype=torch.float16, device=dev)
    nbytes = L.qqq_verify_attn_workspace_bytes(b, t, h, kvh, d, max_len)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev)
    P = ops._ptr
    tail = (P(table), table.shape[1], P(start), float(scale), P(o16), P(xq), P(s1), P(ws), nbytes, b, t, h, kvh, d, nb, bs, max_len,
            dev.index or 0, ops._stream_for(q))
    fn = L.qqq_verify_attn_paged_kv8 if kv8 else L.qqq_verify_attn_paged
    err = fn(*(P(x) for x in (q,) + tuple(pools)), *tail)
    assert err == 0, _lib.last_error()
    torch.cuda.synchronize()
    return xq, s1, o16


def _assert_sentinels(got, rows, what):
    xq, s1, o16 = got
    for r in rows:
        assert bool((o16[r] == SENT).all()) and bool((xq[r] == 77).all()) and float(s1[r]) == SENT, (what, r)


def _verify_against_decode(dev, g, h, kvh, d, t, b, starts, bs, cap, max_len, kv8, what):
    """a chunk of t tokens per row at `starts`, over a pool of cap slots per row whose table is poisoned beyond each row's last block:
    shapes, every in-range token against the decode op, sentinels in every other token, the exact quantiser on the in-range tokens"""
    _, pools, table, poison = _decode_case(dev, g, b, h, kvh, d, cap, bs, kv8)
    q = torch.randn((b * t, h, d), generator=g, device=dev).half()
    start = torch.tensor(starts, dtype=torch.int64, device=dev)
    tab = _poisoned_chunk(table, start, t, bs, poison, max_len)
    last = ((start + t - 1).clamp(0, max_len - 1) // bs).tolist()
    for r in range(b):  # the table the kernel gets names the poison block beyond each row's last block
        assert bool((tab[r, last[r] + 1:] == poison).all()) and bool((tab[r, :last[r] + 1] == table[r, :last[r] + 1]).all())
    got = _verify_lib(q, pools, tab, start, t, d ** -0.5, max_len, kv8)
    assert got[0].shape == (b * t, h * d) and got[1].shape == (b * t, 1) and got[2].shape == (b * t, h * d)
    assert got[0].dtype == torch.int8 and got[1].dtype == torch.float32 and got[2].dtype == torch.float16
    live = [r * t + j for r in range(b) for j in range(t) if starts[r] >= 0 and starts[r] + j < max_len]
    dead = [i for i in range(b * t) if i not in live]
    assert live
    started = [r for r in range(b) if starts[r] >= 0]  # a row with start < 0 writes no token, whatever start + j is
    _assert_tokens_equal_decode(got, q, pools, tab, start, t, d ** -0.5, max_len, kv8, what, rows=started)
    _assert_sentinels(got, dead, what)
    _assert_quant_exact(got[0][live], got[1][live], got[2][live], what)


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("case", VERIFY_CASES, ids=lambda c: "-".join(str(x) for x in c[:4]))
def test_verify_every_token_equals_the_decode_op(dev, case, kv8):
    h, kvh, d, t = case[:4]
    check_verify_case(*case)
    chunk = _chunk(dev, V_B, kvh, V_MAX_LEN)
    splits = -(-V_MAX_LEN // chunk)
    assert chunk % 128 == 0 and splits >= 2
    assert t < 3 or chunk - 2 + t - 1 >= chunk  # the third row's tokens lie on both sides of a split boundary
    print(f"verify h={h} kvh={kvh} d={d} t={t} kv8={kv8}: plan splits={splits} chunk={chunk}")
    g = torch.Generator(device=dev).manual_seed(h * 13 + kvh + t * 5 + d)
    starts = (0, 30, chunk - 2, V_MAX_LEN - t)
    _verify_against_decode(dev, g, h, kvh, d, t, V_B, starts, 16, V_MAX_LEN, V_MAX_LEN, kv8, ("verify", h, kvh, d, t, kv8, chunk))


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("bs", [128, 256])
@pytest.mark.parametrize("h,kvh,d,t", VERIFY_ONE_PER_G)
def test_verify_at_other_block_sizes(dev, h, kvh, d, t, bs, kv8):
    """block_size 128 and 256 (the table reaches 768 keys, a whole number of either): chunks whose tokens lie on both sides of a block
    boundary (start = bs - 2, and 2 * bs - 1 where that is below max_len), in the first block and at the end"""
    assert t >= 3 and (h // kvh) * t <= 64
    cap = 768
    assert cap % bs == 0 and cap >= V_MAX_LEN
    chunk = _chunk(dev, V_B, kvh, V_MAX_LEN)
    print(f"verify h={h} kvh={kvh} d={d} t={t} bs={bs} kv8={kv8}: plan splits={-(-V_MAX_LEN // chunk)} chunk={chunk}")
    g = torch.Generator(device=dev).manual_seed(h * 3 + kvh + t + d + bs)
    starts = (0, bs - 2, min(2 * bs - 1, V_MAX_LEN - t - 1), V_MAX_LEN - t)
    assert (bs - 2) // bs != (bs - 2 + t - 1) // bs
    _verify_against_decode(dev, g, h, kvh, d, t, V_B, starts, bs, cap, V_MAX_LEN, kv8, ("verify block size", h, kvh, d, t, bs, kv8))


@pytest.mark.parametrize("kv8", [False, True])
def test_verify_under_a_plan_of_longer_chunks(dev, kv8):
    """chunk >= 256: b * kvh = 256 workgroups per split leave four planned splits of 640 keys on 256 compute units, chunks of 256 keys
    and a short last one.  Chunks of tokens on both sides of the first and of the second split boundary, and one around key 128, which is
    inside the first split now."""
    h, kvh, d, t = 128, 64, 64, 16
    b = next((n for n in (4, 8, 16, 32, 64) if _chunk(dev, n, kvh, V_MAX_LEN) >= 256), None)
    if b is None:
        pytest.skip(f"no plan with chunks of 256 keys up to b = 64 on this device: chunk {_chunk(dev, 64, kvh, V_MAX_LEN)}")
    chunk = _chunk(dev, b, kvh, V_MAX_LEN)
    splits = -(-V_MAX_LEN // chunk)
    print(f"verify h={h} kvh={kvh} d={d} t={t} b={b} kv8={kv8}: plan splits={splits} chunk={chunk}")
    starts = (chunk - 2, min(2 * chunk - 1, V_MAX_LEN - t - 1), 128 - 2, V_MAX_LEN - t) * (b // 4)
    assert chunk >= 256 and 128 - 2 + t - 1 < chunk and 128 - 2 < 128 <= 128 - 2 + t - 1  # keys 126 ... 141 lie inside one split
    assert splits >= 2 and chunk - 2 < chunk <= chunk - 2 + t - 1
    if splits >= 3:
        assert 2 * chunk - 1 < 2 * chunk <= 2 * chunk - 1 + t - 1 < V_MAX_LEN and V_MAX_LEN - (splits - 1) * chunk < chunk  # a short last split
    g = torch.Generator(device=dev).manual_seed(97 + b)
    _verify_against_decode(dev, g, h, kvh, d, t, b, starts, 16, V_MAX_LEN, V_MAX_LEN, kv8, ("verify long chunks", b, chunk, kv8))


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("h,kvh,d,t", [(24, 8, 128, 11), (40, 8, 128, 12), (96, 16, 128, 3)])
def test_verify_with_a_max_len_that_is_no_multiple_of_the_chunk(dev, h, kvh, d, t, kv8):
    """max_len = 600 over a table that reaches 640: the last split is a short one.  A row whose first two tokens alone are below max_len
    (the others write nothing), a row across the last split boundary, a retired row and a row that starts at max_len."""
    max_len, cap = 600, 640
    chunk = _chunk(dev, V_B, kvh, max_len)
    splits = -(-max_len // chunk)
    print(f"verify h={h} kvh={kvh} d={d} t={t} max_len={max_len} kv8={kv8}: plan splits={splits} chunk={chunk}")
    assert max_len % chunk != 0 and t >= 3
    if chunk == 128:
        assert max_len - (splits - 1) * chunk == 88 and 511 < 512 <= 511 + t - 1
    g = torch.Generator(device=dev).manual_seed(h + kvh * 7 + t + d)
    _verify_against_decode(dev, g, h, kvh, d, t, V_B, (598, 511, -1, 600), 16, cap, max_len, kv8, ("verify max_len 600", h, kvh, d, t, kv8))


def _kv64(pools, table, kv8):
    if kv8:
        return (K8.dequant64(_from_pool(pools[0], table), _from_pool(pools[2], table)),
                K8.dequant64(_from_pool(pools[1], table), _from_pool(pools[3], table)))
    return _from_pool(pools[0], table), _from_pool(pools[1], table)


@pytest.mark.parametrize("kv8", [False, True])
def test_verify_against_float64_at_five_rows_per_token(dev, kv8):
    """The absolute anchor at G = 5, 60 query rows: relative L2 per (token, head) <= 1e-3 and max error <= 2^-9 max|v| over the keys
    attended, the bounds and the float64 reference of tests/test_gpu_decode_attn.py.  Observed on an MI355X (chunk 128): fp16 pool rel L2 3.42e-04,
    max 2.26e-04; int8 pool 4.81e-04, 4.91e-04."""
    h, kvh, d, t = 40, 8, 128, 12
    chunk = _chunk(dev, V_B, kvh, V_MAX_LEN)
    g = torch.Generator(device=dev).manual_seed(53)
    _, pools, table, poison = _decode_case(dev, g, V_B, h, kvh, d, V_MAX_LEN, 16, kv8)
    q = torch.randn((V_B * t, h, d), generator=g, device=dev).half()
    start = torch.tensor((0, 30, chunk - 2, V_MAX_LEN - t), dtype=torch.int64, device=dev)
    got = _verify_lib(q, pools, _poisoned_chunk(table, start, t, 16, poison, V_MAX_LEN), start, t, d ** -0.5, V_MAX_LEN, kv8)
    k64, v64 = _kv64(pools, table, kv8)
    o = got[2].reshape(V_B, t, h * d)
    q4 = q.reshape(V_B, t, h, d)
    worst = (0.0, 0.0)
    for j in range(t):
        pos = start + j
        qj = q4[:, j, :, None].contiguous()
        ref = K8.attention64(qj, k64, v64, pos, d ** -0.5) if kv8 else _ref64(qj, k64, v64, pos, d ** -0.5)
        rel, mx = _errors(o[:, j].contiguous(), ref, v64, pos)
        worst = (max(worst[0], rel), max(worst[1], mx))
    print(f"verify_attention_paged{'_kv8' if kv8 else ''} h={h} kvh={kvh} d={d} t={t} chunk={chunk} vs float64: rel L2 {worst[0]:.2e}, "
          f"max|err|/max|v| {worst[1]:.2e} (2^-9 = {2 ** -9:.2e})")
    assert worst[0] <= 1e-3 and worst[1] <= 2 ** -9, worst


# ---- the shared prefix

#               h, kvh,   d, pack: the packs min(family_max, 64 // G) of a large family (21 at G = 3, 12 at G = 5, 9 at G = 7), and small ones
SHARED_CASES = [(16, 8, 64, 16), (24, 8, 128, 21), (24, 8, 128, 11), (33, 11, 128, 5), (40, 8, 128, 12), (40, 8, 128, 3), (96, 16, 64, 10),
                (28, 4, 128, 9), (64, 8, 128, 8), (65, 13, 128, 4), (128, 16, 128, 2)]


def shared_lengths(chunk, max_len=SH.MAX_LEN):
    """no prefix, one that ends inside the first split (nothing joint), exactly one split, one split and a half (the second split ends
    outside the prefix and is private for every member), and three splits -- or as many whole splits as leave keys behind the prefix
    below max_len, where the plan's chunks are longer than a quarter of max_len"""
    return [0, chunk // 2, chunk, chunk + chunk // 2, min(3 * chunk, (max_len - 1) // chunk * chunk)]


def shared_batch(pack):
    return 2 * pack + 4


def shared_calls(pack, chunk, max_len=SH.MAX_LEN):
    """Five calls of b = 2 * pack + 4 rows: a family of pack + 1 (two packs, the second of one row), a lone row, a family of exactly pack
    and one of two.  Over the five calls every family size meets every shared length.  Members stand at SH._positions relative to the
    prefix.  One member of each large family stands half a chunk and three keys below its family's prefix: what it shares is clamped to
    its own keys, which takes it out of the last split its siblings take jointly.  In the family of pack + 1 it is the second member of
    the first pack (the first where pack is 2), which leaves a hole in the live set; in the family of pack it is the last, which shortens
    the live set.  The second member of the family of pack is retired (pos = -1).
    -> [(families for SH._case, retired rows)]"""
    cg = torch.Generator().manual_seed(pack)
    lens = shared_lengths(chunk, max_len)
    below = lambda s: max(s - chunk // 2 - 3, 0)
    calls = []
    for c in range(5):
        big, mid, two = lens[c], lens[(c + 2) % 5], lens[(c + 4) % 5]
        p_big = SH._positions(cg, pack + 1, big, chunk)
        p_big[1 if pack >= 3 else 0] = below(big)
        p_mid = SH._positions(cg, pack, mid, chunk)
        p_mid[1] = -1
        if pack >= 3:
            p_mid[pack - 1] = below(mid)
        lone = [int(torch.randint(0, max_len, (1,), generator=cg))]
        fams = [(pack + 1, big, p_big), (1, 0, lone), (pack, mid, p_mid), (2, two, SH._positions(cg, 2, two, chunk))]
        assert all(-1 <= p < max_len for _, _, ps in fams for p in ps)
        calls.append((fams, [pack + 1 + 1 + 1]))
    return calls


def descriptors(fams):
    """family, shared, pos of SH._case as Python lists"""
    family, shared, pos, r = [], [], [], 0
    for size, s, ps in fams:
        family += [r] * size
        shared += [s if size > 1 else 0] * size
        pos += ps
        r += size
    return family, shared, pos


def check_shared_case(h, kvh, pack, splits, chunk, max_len=SH.MAX_LEN):
    """What the calls of a case put through the kernel under the plan (splits, chunk), by the model of tests/shared_ref.py.  Returns the
    calls.  Over the case's calls together:
      - some job has two or more live slots, and some job's live set has a hole;
      - some split begins inside a family's prefix and ends outside it, and every member takes that split alone;
      - where G does not divide 16 and the pack has more than 16 query rows (so that a slot can straddle at all), some joint job has a
        live slot whose G rows lie in two tiles;
      - where the instantiation has more than one tile, some joint job ends before the last tile, which is then skipped (a private job
        always does);
      - every row of every job is below b, every row in range has every split up to its pos written exactly once, and nothing else is."""
    G = h // kvh
    b = shared_batch(pack)
    assert h % kvh == 0 and G * pack <= 64 and splits * chunk >= max_len > (splits - 1) * chunk and 2 * chunk < max_len
    nq = REF.tiles(pack, G)
    joint, holes, partly, straddle, skipped = 0, 0, 0, 0, 0
    calls = shared_calls(pack, chunk, max_len)
    for fams, retired in calls:
        family, shared, pos = descriptors(fams)
        assert len(pos) == b and all(pos[r] == -1 for r in retired)
        jobs = REF.jobs(family, shared, pos, pack, chunk, splits, max_len, G)
        written = {}
        for job in jobs:
            assert all(0 <= r < b for r in REF.covered(job)) and REF.query_rows(job, G) <= 16 * nq
            for r in REF.covered(job):
                written[(r, job.split)] = written.get((r, job.split), 0) + 1
            many = len(job.live) >= 2
            joint += many
            holes += REF.has_hole(job)
            straddle += many and bool(REF.straddling_slots(job, G))
            skipped += many and REF.query_rows(job, G) <= 16 * (nq - 1)
        want = {(r, sp) for r in range(b) if 0 <= pos[r] < max_len for sp in range(splits) if sp * chunk <= pos[r]}
        assert set(written) == want and set(written.values()) == {1}
        r0 = 0
        for size, s, _ in fams:
            rows = range(r0, r0 + size)
            r0 += size
            if size > 1 and s % chunk:
                sp = s // chunk  # begins inside the prefix, ends outside it
                mine = [j for j in jobs if j.split == sp and set(REF.covered(j)) & set(rows)]
                assert all(j.live == (0,) for j in mine)
                partly += len(mine) >= 2
    assert joint and holes and partly, (joint, holes, partly)
    if 16 % G != 0 and G * pack > 16:
        assert straddle, (G, pack)
    if nq > 1:
        assert skipped, (G, pack)
    return calls


def _run_shared_case(dev, h, kvh, d, pack, bs, kv8, calls, what):
    g = torch.Generator(device=dev).manual_seed(h * 7 + kvh * 3 + pack + d + bs)
    b = shared_batch(pack)
    for fams, retired in calls:
        # with block_size 16 every prefix is a whole number of blocks; with 256 most end inside a block, which is then a block of each
        # sibling's own whose leading rows are copies
        pools, table, pos, family, shared = SH._case(dev, g, fams, bs, kvh, d, kv8, whole_blocks=bs == 16)
        assert pos.numel() == b
        q = torch.randn((b, h, d), generator=g, device=dev).half()
        want = SH._plain(q, pools, table, pos, d ** -0.5, kv8)
        got = SH._shared(q, pools, table, pos, family, shared, pack, d ** -0.5, kv8)
        SH._assert_rows_equal(got, want, pos, (what, [(n, s) for n, s, _ in fams]), untouched=retired)


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("bs", [16, 256])
@pytest.mark.parametrize("h,kvh,d,pack", SHARED_CASES)
def test_shared_every_row_equals_the_plain_op(dev, h, kvh, d, pack, bs, kv8):
    from qqq_amd import ops

    splits, chunk = ops.decode_attention_shared_plan(shared_batch(pack), h, kvh, SH.MAX_LEN, pack)
    print(f"shared h={h} kvh={kvh} d={d} pack={pack} b={shared_batch(pack)} bs={bs} kv8={kv8}: plan splits={splits} chunk={chunk}")
    calls = check_shared_case(h, kvh, pack, splits, chunk)
    _run_shared_case(dev, h, kvh, d, pack, bs, kv8, calls, ("shared", h, kvh, d, pack, bs, kv8, chunk))


PARTIAL = {16: 200, 256: 384}  # block_size: a prefix that ends inside a block, and behind the first 128-key split


def partial_families(pack, bs):
    s = PARTIAL[bs]
    cg = torch.Generator().manual_seed(pack + bs)
    return [(pack + 1, s, SH._positions(cg, pack + 1, s)), (1, 0, [s + 40]), (2, s, SH._positions(cg, 2, s))]


def check_partial_case(h, kvh, pack, bs, splits, chunk):
    """the prefix ends inside a block (with block_size 16 inside a split of 128 keys too): shared // 128 splits are taken jointly, and with
    block_size 256 the last of them lies in the block that every sibling holds a copy of"""
    s = PARTIAL[bs]
    assert chunk == 128 and splits == SH.MAX_LEN // 128 and s % bs != 0 and s // chunk >= 1 and (bs != 16 or s % chunk != 0)
    if bs == 256:
        assert (s // chunk * chunk - 1) // bs == s // bs  # the last joint split lies in the copied block
    fams = partial_families(pack, bs)
    family, shared, pos = descriptors(fams)
    jobs = REF.jobs(family, shared, pos, pack, chunk, splits, SH.MAX_LEN, h // kvh)
    assert max(j.split for j in jobs if len(j.live) >= 2) == s // chunk - 1
    assert all(j.row == j.base + j.live[0] for j in jobs)  # the first live member computes
    return fams


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("bs", [16, 256])
@pytest.mark.parametrize("h,kvh,d,pack", [(24, 8, 128, 11), (64, 8, 128, 4)])
def test_shared_prefix_that_ends_inside_a_block(dev, h, kvh, d, pack, bs, kv8):
    """`shared` counts keys; the tables must agree on the first shared // block_size blocks only.  The block that holds the end of the
    prefix is a copy of each sibling's own with the same leading rows, as copy-on-write of a partial block leaves it."""
    from qqq_amd import ops

    b = pack + 4
    splits, chunk = ops.decode_attention_shared_plan(b, h, kvh, SH.MAX_LEN, pack)
    print(f"shared partial block h={h} kvh={kvh} d={d} pack={pack} b={b} bs={bs} kv8={kv8}: plan splits={splits} chunk={chunk}")
    fams = check_partial_case(h, kvh, pack, bs, splits, chunk)
    g = torch.Generator(device=dev).manual_seed(h + kvh + pack + bs)
    pools, table, pos, family, shared = SH._case(dev, g, fams, bs, kvh, d, kv8, whole_blocks=False)
    root_blocks, sib_blocks = table[0], table[1]
    n = PARTIAL[bs] // bs
    assert torch.equal(root_blocks[:n], sib_blocks[:n]) and int(root_blocks[n]) != int(sib_blocks[n])
    q = torch.randn((b, h, d), generator=g, device=dev).half()
    want = SH._plain(q, pools, table, pos, d ** -0.5, kv8)
    got = SH._shared(q, pools, table, pos, family, shared, pack, d ** -0.5, kv8)
    SH._assert_rows_equal(got, want, pos, ("shared partial block", h, kvh, d, pack, bs, kv8))


@pytest.mark.parametrize("kv8", [False, True])
def test_shared_against_float64_at_packs_of_21(dev, kv8):
    """The absolute anchor at G = 3 and the pack of 21 siblings fuse_shared() passes for Llama-3.2-3B, 63 query rows: the bounds and the
    float64 reference of tests/test_gpu_decode_attn.py over every live row of the case's calls.  Observed on an MI355X (three splits of 384 keys): fp16 pool
    rel L2 3.31e-04, max 1.75e-04; int8 pool 4.23e-04, 4.05e-04."""
    from qqq_amd import ops

    h, kvh, d, pack, bs = 24, 8, 128, 21, 16
    b = shared_batch(pack)
    splits, chunk = ops.decode_attention_shared_plan(b, h, kvh, SH.MAX_LEN, pack)
    calls = check_shared_case(h, kvh, pack, splits, chunk)
    g = torch.Generator(device=dev).manual_seed(61)
    worst = (0.0, 0.0)
    for fams, retired in calls[3:]:  # the calls with the two longest prefixes in the family of two packs
        pools, table, pos, family, shared = SH._case(dev, g, fams, bs, kvh, d, kv8)
        q = torch.randn((b, h, d), generator=g, device=dev).half()
        got = SH._shared(q, pools, table, pos, family, shared, pack, d ** -0.5, kv8)
        live = torch.tensor([r for r in range(b) if r not in retired], device=dev)
        tl = table[live].long()
        k64, v64 = _kv64(pools, tl, kv8)
        ql = q[live][:, :, None].contiguous()
        ref = K8.attention64(ql, k64, v64, pos[live], d ** -0.5) if kv8 else _ref64(ql, k64, v64, pos[live], d ** -0.5)
        rel, mx = _errors(got[2][live], ref, v64, pos[live])
        worst = (max(worst[0], rel), max(worst[1], mx))
    print(f"decode_attention_paged_shared{'_kv8' if kv8 else ''} h={h} kvh={kvh} d={d} pack={pack} splits={splits} chunk={chunk} vs float64: "
          f"rel L2 {worst[0]:.2e}, max|err|/max|v| {worst[1]:.2e} (2^-9 = {2 ** -9:.2e})")
    assert worst[0] <= 1e-3 and worst[1] <= 2 ** -9, worst
