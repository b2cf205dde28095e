"""GPTQ with act-order and static groups on the GPU: the two HIP ops (ops.gptq_block_cols, ops.group_scales) against the CPU restatement
tests/gptq_order_ref.py and against the ops they generalise, bit for bit; gptq_quantize_ordered block by block through its trace; packing;
and quantize_model(act_order=True, static_groups=True) over the small model of tests/test_gpu_gptq_model.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gptq_order_ref as O
import gptq_ref as R

pytestmark = pytest.mark.gpu

K_FACTOR = 384
GROUPS = 3
ROWS_PADS = ((1, (0, 0, 0)), (63, (5, 0, 3)), (64, (0, 7, 0)), (65, (1, 2, 3)), (200, (64, 128, 8)))


def _calibration(seed, K, rows=512):
    rng = np.random.Generator(np.random.PCG64(seed))
    mix = rng.standard_normal((K, K)) * (rng.random((K, K)) < 0.05) + np.eye(K)
    X = (rng.standard_normal((rows, K)) * (0.2 + rng.random(K) * 2)) @ mix
    return (2.0 / 4 * X.T @ X).astype(np.float32)


@pytest.fixture(scope="module")
def factor():
    """a 384 x 384 upper factor (CPU Cholesky chain of a correlated Hessian), 200 weight rows and their three groups' scales; shared and
    never modified"""
    Hinv, _ = R.hinv_of(_calibration(3, K_FACTOR))
    W = (np.random.Generator(np.random.PCG64(4)).standard_normal((200, K_FACTOR)) * 0.02).astype(np.float32)
    W[:, 128:256] *= 3  # three groups of clearly different scales
    W[:, 256:] *= 0.4
    return Hinv, W, O.group_scales(W)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def gidx_pattern(kind, count):
    i = np.arange(count)
    if kind == "constant":
        g = np.full(count, 2)
    elif kind == "alternating":
        g = i % 2
    elif kind == "random":
        g = np.random.Generator(np.random.PCG64(count)).integers(0, GROUPS, count)
    else:  # "seams": the group changes inside a lane's four columns (between its second and third) and at every 32-column chunk seam
        g = ((i % 4 >= 2) + 2 * (i // 32)) % GROUPS
    return g.astype(np.int32)


def _gpu_block_cols(W1, Hinv_full, off, count, S, gidx, pad=(0, 0, 0)):
    """the op on views: W1 inside a wider matrix, Hinv1 a block of the full factor (ldh = 384), scales a column range of a five-column
    table (lds = 5 > groups), Q1 / Err1 inside wider outputs; everything around them is a sentinel"""
    from qqq_amd.quant import ops

    dev = torch.device("cuda:0")
    rows, groups = W1.shape[0], S.shape[1]
    Wd = torch.full((rows, count + pad[0]), float("nan"), device=dev)
    Wd[:, :count] = torch.from_numpy(W1).to(dev)
    Hd = torch.from_numpy(Hinv_full).to(dev)
    Sd = torch.full((rows, groups + 2), float("nan"), device=dev)
    Sd[:, 1:1 + groups] = torch.from_numpy(S).to(dev)
    gd = torch.from_numpy(gidx).to(dev)
    Qd = torch.full((rows, count + pad[1]), 123.0, device=dev)
    Ed = torch.full((rows, count + pad[2]), 456.0, device=dev)
    before = Wd.clone()
    ops.gptq_block_cols(Wd[:, :count], Hd[off:off + count, off:off + count], Sd[:, 1:1 + groups], gd, out=(Qd[:, :count], Ed[:, :count]))
    torch.cuda.synchronize()
    assert torch.equal(Wd[:, :count], before[:, :count])  # W1 is read only
    assert (Qd[:, count:] == 123.0).all() and (Ed[:, count:] == 456.0).all()  # the padding is not touched
    assert torch.equal(gd.cpu(), torch.from_numpy(gidx))
    return Qd[:, :count].cpu().numpy(), Ed[:, :count].cpu().numpy()


@pytest.mark.parametrize("kind", ["constant", "alternating", "random", "seams"])
@pytest.mark.parametrize("count", [64, 128])
def test_block_cols_is_the_restatement_bit_for_bit(factor, count, kind):
    Hinv, W, S = factor
    off = 128 if count == 128 else 320  # a block on the diagonal of the 384 x 384 factor: ldh = 384
    gidx = gidx_pattern(kind, count)
    if kind == "seams":
        assert all(len(set(gidx[j:j + 4].tolist())) == 2 for j in range(0, count, 4)) and all(gidx[j - 1] != gidx[j] for j in range(32, count, 32))
    for rows, pad in ROWS_PADS:
        W1 = W[:rows, off:off + count].copy()
        want_q, want_e = O.block_cols(W1, Hinv[off:off + count, off:off + count], S[:rows][:, gidx])
        got_q, got_e = _gpu_block_cols(W1, Hinv, off, count, S[:rows], gidx, pad)
        assert np.array_equal(_bits(got_q), _bits(want_q)), (rows, pad)
        assert np.array_equal(_bits(got_e), _bits(want_e)), (rows, pad)


@pytest.mark.parametrize("count", [64, 128])
def test_block_cols_with_a_constant_group_is_gptq_block(factor, count):
    from qqq_amd.quant import ops

    Hinv, W, S = factor
    dev = torch.device("cuda:0")
    off = 0 if count == 128 else 64
    Hd = torch.from_numpy(Hinv).to(dev)[off:off + count, off:off + count]
    for rows in (1, 65, 200):
        Wd, Sd = torch.from_numpy(W[:rows, off:off + count].copy()).to(dev), torch.from_numpy(S[:rows].copy()).to(dev)
        for g in range(GROUPS):
            want_q, want_e = ops.gptq_block(Wd, Hd, Sd[:, g].contiguous(), True)
            got_q, got_e = ops.gptq_block_cols(Wd, Hd, Sd, torch.full((count,), g, dtype=torch.int32, device=dev))
            assert torch.equal(got_q.view(torch.int32), want_q.view(torch.int32)), (rows, g)
            assert torch.equal(got_e.view(torch.int32), want_e.view(torch.int32)), (rows, g)


def _crafted(count):
    """seven rows whose neighbouring columns sit under different scales (gidx alternates 0, 1) -> (W, scales [7, 2], gidx)"""
    rng = np.random.Generator(np.random.PCG64(9))
    gidx = (np.arange(count) % 2).astype(np.int32)
    W = np.zeros((7, count), np.float32)
    S = np.ones((7, 2), np.float32)
    # 0: an all-zero row under the scale an all-zero group gets, and another
    S[0] = np.float32(2) / np.float32(15), np.float32(0.25)
    # 1, 2: power-of-two scales, weights on exact .5 ties of their own column's scale (both parities, both signs)
    S[1], S[2] = (0.25, 0.5), (2.0 ** -10, 2.0 ** -9)
    W[1] = (rng.integers(-9, 9, count) + 0.5) * S[1][gidx]
    W[2] = (rng.integers(-9, 9, count) + 0.5) * S[2][gidx]
    # 3, 4: far outside the clamp on both sides
    W[3] = np.where(rng.random(count) < 0.5, 1e3, -1e3) * (1 + rng.random(count))
    W[4] = np.where(rng.random(count) < 0.5, 1e20, -1e20)
    S[3], S[4] = (0.01, 0.02), (1e15, 2e15)
    # 5: subnormal weights under ordinary scales;  6: subnormal weights under subnormal scales
    W[5] = (rng.integers(-50, 50, count) * 1e-42).astype(np.float32)
    W[6] = W[5]
    own = R.scales(W[6:7], True)[0]
    S[5], S[6] = (0.01, 0.02), (own, own + own)
    return W.astype(np.float32), S, gidx


@pytest.mark.parametrize("count", [64, 128])
def test_block_cols_crafted_rows(factor, count):
    Hinv = factor[0]
    off = 0 if count == 128 else 64
    W1, S, gidx = _crafted(count)
    tiny = np.finfo(np.float32).tiny
    assert np.abs(W1[5]).max() < tiny and 0 < S[6].min() and S[6].max() < tiny
    k = np.rint(W1[1, :2] / S[1] - 0.5)
    assert np.array_equal(k + 0.5, W1[1, :2] / S[1])  # exact ties
    want_q, want_e = O.block_cols(W1, Hinv[off:off + count, off:off + count], S[:, gidx])
    got_q, got_e = _gpu_block_cols(W1, Hinv, off, count, S, gidx)
    for r in range(W1.shape[0]):
        assert np.array_equal(_bits(got_q[r]), _bits(want_q[r])), r
        assert np.array_equal(_bits(got_e[r]), _bits(want_e[r])), r
    assert not got_q[0].any() and not got_e[0].any()
    codes = np.rint(got_q[3] / S[3][gidx]) + 8
    assert codes.min() == 0 and codes.max() == 15  # the clamp holds on both sides


def test_block_cols_clamps_the_group_index(factor):
    Hinv, W, S = factor
    gidx = gidx_pattern("random", 128)
    wild = gidx.copy()
    wild[gidx == 0] = -1
    wild[gidx == GROUPS - 1] = GROUPS
    wild[5], wild[70] = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    clamped = np.clip(wild, 0, GROUPS - 1).astype(np.int32)
    assert (wild == -1).any() and (wild == GROUPS).any()
    W1 = W[:65, :128].copy()
    want_q, want_e = _gpu_block_cols(W1, Hinv, 0, 128, S[:65], clamped)
    got_q, got_e = _gpu_block_cols(W1, Hinv, 0, 128, S[:65], wild)  # the table's neighbours are NaN: a read outside the range would show
    assert np.array_equal(_bits(got_q), _bits(want_q)) and np.array_equal(_bits(got_e), _bits(want_e))
    ref_q, ref_e = O.block_cols(W1, Hinv[:128, :128], S[:65][:, clamped])
    assert np.array_equal(_bits(got_q), _bits(ref_q)) and np.array_equal(_bits(got_e), _bits(ref_e))


def test_block_cols_rows_do_not_know_their_place_and_graph_replay_gives_the_eager_bits(factor):
    from qqq_amd.quant import ops

    Hinv, W, S = factor
    dev = torch.device("cuda:0")
    gidx = gidx_pattern("random", 128)
    alone_q, alone_e = _gpu_block_cols(W[:41, :128].copy(), Hinv, 0, 128, S[:41], gidx)
    big_w, big_s = np.roll(W[:, :128], 77, axis=0).copy(), np.roll(S, 77, axis=0).copy()  # the same rows at offset 77 of a 200-row launch
    big_q, big_e = _gpu_block_cols(big_w, Hinv, 0, 128, big_s, gidx)
    assert np.array_equal(_bits(big_q[77:118]), _bits(alone_q)) and np.array_equal(_bits(big_e[77:118]), _bits(alone_e))
    # a captured launch replays with other contents of the same buffers: W1, scales AND gidx
    Wd, Hd, Sd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (W[:, :128], Hinv[:128, :128], S))
    gd = torch.from_numpy(gidx).to(dev)
    out = (torch.empty((200, 128), device=dev), torch.empty((200, 128), device=dev))
    ops.gptq_block_cols(Wd, Hd, Sd, gd, out=out)  # warm-up outside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.gptq_block_cols(Wd, Hd, Sd, gd, out=out)
    other = gidx_pattern("seams", 128)
    assert (other != gidx).any()
    for w_np, s_np, g_np in ((big_w, big_s, other), (W[:, :128], S, gidx)):
        Wd.copy_(torch.from_numpy(np.ascontiguousarray(w_np)))
        Sd.copy_(torch.from_numpy(np.ascontiguousarray(s_np)))
        gd.copy_(torch.from_numpy(g_np))
        out[0].zero_()
        g.replay()
        torch.cuda.synchronize()
        want_q, want_e = _gpu_block_cols(np.ascontiguousarray(w_np), Hinv, 0, 128, np.ascontiguousarray(s_np), g_np)
        assert np.array_equal(_bits(out[0].cpu().numpy()), _bits(want_q)) and np.array_equal(_bits(out[1].cpu().numpy()), _bits(want_e))


def _scale_rows(rows, cols, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    W = (rng.standard_t(3, size=(rows, cols)) * 0.01).astype(np.float32)  # heavy tails: the shrink search moves
    W[1] = 0  # an all-zero row
    if cols > 128:
        W[2, 128:256] = 0  # an all-zero group inside a live row
    return W


@pytest.mark.parametrize("rows,cols", [(37, 128), (37, 384), (5, 4096), (3, 11008)])
def test_group_scales_are_the_restatement_and_weight_scales_per_group(rows, cols):
    from qqq_amd.quant import ops

    W = _scale_rows(rows, cols, cols)
    wide = np.full((rows, cols + 5), np.nan, np.float32)  # a column slice of a wider matrix
    wide[:, :cols] = W
    Wd = torch.from_numpy(wide).cuda()[:, :cols]
    G = cols // 128
    chosen = set()
    for mse in (False, True):
        got = ops.group_scales(Wd, mse)
        assert got.shape == (rows, G) and got.dtype == torch.float32 and got.is_contiguous()
        per_group = torch.cat([ops.weight_scales(Wd[:, 128 * g:128 * g + 128], True, mse) for g in range(G)], dim=1)
        assert torch.equal(got.view(torch.int32), per_group.view(torch.int32)), mse
        got = got.cpu().numpy()
        if not mse:
            assert np.array_equal(_bits(got), _bits(O.group_scales(W)))
            assert got[1, 0] == np.float32(2) / np.float32(15) and (cols == 128 or got[2, 1] == np.float32(2) / np.float32(15))
        else:
            for g in range(G):
                cand = R.candidates(W[:, 128 * g:128 * g + 128], True)
                for r in range(rows):
                    hit = np.flatnonzero(_bits(cand[r]) == _bits(got[r:r + 1, g]))
                    assert hit.size, (r, g)  # a candidate's scale, bit for bit
                    chosen.add(int(hit[0]))
    print(f"group_scales {rows} x {cols}: shrink candidates chosen {sorted(chosen)}")
    assert len(chosen) > 2


TRACE_N, TRACE_K, TRACE_DEAD = 200, 384, 77
TRACE_SEED = 11
# the proxy loss tr((W - Q) H (W - Q)^T) of the CPU restatement (sweep_ordered, act-order + static groups) on the trace input with the
# trailing GEMM in f32 and in f64, over the input seeds 11 ... 18: the relative spread is 0, 0, 0, 0, 0, 0, 0, 0 per-channel and
# 0, 0, 0, 0, 0, 0, 0, 0 with g128 -- the static scales do not see the GEMM, and at none of the seeds does its rounding flip a code.  The
# allowed difference is 10 x the largest of the eight: 0.  The GPU's loss must be the restatement's on the GPU's own factor.
LOSS_SPREAD = {-1: 0.0, 128: 0.0}


def trace_inputs(seed=TRACE_SEED):
    """test_gpu_gptq.py's trace input: an fp16 weight and the Hessian of 512 correlated calibration rows in four samples, one column dead"""
    rng = np.random.Generator(np.random.PCG64(seed))
    W = (rng.standard_normal((TRACE_N, TRACE_K)) * 0.02).astype(np.float16)
    mix = rng.standard_normal((TRACE_K, TRACE_K)) * (rng.random((TRACE_K, TRACE_K)) < 0.05) + np.eye(TRACE_K)
    X = (rng.standard_normal((512, TRACE_K)) * (0.2 + rng.random(TRACE_K) * 2)) @ mix
    X[:, TRACE_DEAD] = 0
    return W, (2.0 / 4 * X.T @ X).astype(np.float32)


@pytest.fixture(scope="module")
def trace_input():
    return trace_inputs()


def _same_result(a, b):
    same = torch.equal(a.weight.view(torch.int16), b.weight.view(torch.int16)) and torch.equal(a.scales.view(torch.int32), b.scales.view(torch.int32))
    same = same and (a.s_extra is None) == (b.s_extra is None) and (a.s_extra is None or torch.equal(a.s_extra, b.s_extra))
    return same and (a.perm is None) == (b.perm is None) and (a.perm is None or torch.equal(a.perm, b.perm))


def _check_trace(res, W, H, perm, grouped):
    """every traced block is the restatement's sweep of its own input, factor block and scales, bit for bit, and its input is the state
    in exact arithmetic within the accumulated bound of the f32 updates before it (test_gptq_quantize_block_by_block's bound)
    -> Q in the swept order"""
    Hinv = res.Hinv.cpu().numpy()
    Wz = W.astype(np.float32)
    Wz[:, np.diag(H) == 0] = 0
    S = O.group_scales(Wz) if grouped else R.scales(W.astype(np.float32), False)[:, None]
    assert len(res.trace) == 3 and [b.start for b in res.trace] == [0, 128, 256]
    state = Wz.astype(np.float64)[:, perm]
    slack = np.zeros_like(state)
    for b in res.trace:
        i1, i2 = b.start, b.start + 128
        block_in, Q1, Err1, scale = (t.cpu().numpy() for t in (b.block_in, b.Q1, b.Err1, b.scale))
        if grouped:
            assert scale.shape == (TRACE_N, 128) and np.array_equal(_bits(scale), _bits(S[:, perm[i1:i2] // 128])), i1
            want_q, want_e = O.block_cols(block_in, Hinv[i1:i2, i1:i2], scale)
        else:
            assert np.array_equal(_bits(scale), _bits(S)), i1
            want_q, want_e = R.block(block_in, Hinv[i1:i2, i1:i2], scale, False)
        assert np.array_equal(_bits(Q1), _bits(want_q)) and np.array_equal(_bits(Err1), _bits(want_e)), i1
        ulp = np.abs(block_in) * 2.0 ** -23 + 2.0 ** -149
        assert (np.abs(block_in - state[:, i1:i2]) <= slack[:, i1:i2] + ulp).all(), i1
        upd = Err1.astype(np.float64) @ Hinv[i1:i2, i2:].astype(np.float64)
        state[:, i2:] -= upd
        slack[:, i2:] += 128 * 2.0 ** -23 * (np.abs(Err1).astype(np.float64) @ np.abs(Hinv[i1:i2, i2:]).astype(np.float64)) + \
            np.abs(state[:, i2:]) * 2.0 ** -23
    assert np.array_equal(res.trace[0].block_in.cpu().numpy(), Wz[:, perm[:128]])  # the first block is the permuted weight itself
    Qp = torch.cat([b.Q1 for b in res.trace], dim=1)
    assert torch.equal(res.weight[:, torch.from_numpy(perm).to(res.weight.device)].view(torch.int16), Qp.to(res.weight.dtype).view(torch.int16))
    assert not res.weight[:, TRACE_DEAD].any()
    assert np.array_equal(_bits(res.scales.cpu().numpy()), _bits(S))  # static groups do not see the GEMM's rounding
    return Qp.cpu().numpy()


@pytest.mark.parametrize("gs", [-1, 128])
def test_gptq_quantize_ordered_block_by_block(trace_input, gs):
    """act_order + static_groups through the trace; fused and composed give the same bits; an explicit perm is honoured; the result
    beats round-to-nearest under the same scales and has the loss of the CPU restatement on the GPU's own factor (margin above).
    Measured on an MI355X: per-channel 0.2179 x round-to-nearest, loss 1156.638718 against the restatement's 1156.638718, no code differs
    (relative difference 0, allowed 0), 0.6845 x the loss of natural order under the same scales (1689.852382); g128 0.2241 x, loss
    845.765800 against 845.765800, no code differs, 0.6982 x natural order under the same static scales (1211.294515).  The composed path
    was run-to-run deterministic."""
    from qqq_amd.quant import gptq_quantize, gptq_quantize_ordered

    W, H = trace_input
    dev = torch.device("cuda:0")
    grouped = gs != -1
    Wd, Hd = torch.from_numpy(W).to(dev), torch.from_numpy(H).to(dev)
    res = gptq_quantize_ordered(Wd, Hd, gs, trace=True)
    assert Hd.cpu().numpy()[TRACE_DEAD, TRACE_DEAD] == 0 and torch.equal(Hd, torch.from_numpy(H).to(dev))  # H is not modified
    d = np.diag(H).copy()
    d[d == 0] = 1
    perm = np.argsort(-d, kind="stable")  # the stable descending order, computed here
    assert res.perm.dtype == torch.int64 and np.array_equal(res.perm.cpu().numpy(), perm)
    if grouped:
        assert all(len(set((perm[i:i + 128] // 128).tolist())) == 3 for i in range(0, TRACE_K, 128))  # every block mixes the groups
    Qp = _check_trace(res, W, H, perm, grouped)
    assert (res.s_extra is None) == (not grouped) and res.loss > 0 and np.isfinite(res.loss)

    # the composed path: run to run first, then against the fused one
    c1, c2 = gptq_quantize_ordered(Wd, Hd, gs, fused=False, trace=True), gptq_quantize_ordered(Wd, Hd, gs, fused=False)
    deterministic = _same_result(c1, c2)
    print(f"gs {gs}: the composed path is run-to-run deterministic: {deterministic}")
    assert deterministic
    assert _same_result(res, c1)
    for a, b in zip(res.trace, c1.trace):
        assert torch.equal(a.Q1.view(torch.int32), b.Q1.view(torch.int32)) and torch.equal(a.Err1.view(torch.int32), b.Err1.view(torch.int32))

    # an explicit order is honoured
    mine = np.random.Generator(np.random.PCG64(5)).permutation(TRACE_K)
    r2 = gptq_quantize_ordered(Wd, Hd, gs, perm=torch.from_numpy(mine), trace=True)
    assert np.array_equal(r2.perm.cpu().numpy(), mine)
    _check_trace(r2, W, H, mine, grouped)
    with pytest.raises(RuntimeError, match="not a permutation"):
        gptq_quantize_ordered(Wd, Hd, gs, perm=torch.zeros(TRACE_K, dtype=torch.int64))

    # the proxy loss, in f64, of the f32 codes
    Wz = W.astype(np.float32)
    Wz[:, TRACE_DEAD] = 0
    Qg = Qp[:, np.argsort(perm)]
    scales = res.scales.cpu().numpy()
    rtn = R.quantise(Wz, np.repeat(scales, 128, axis=1) if grouped else scales, grouped)
    ref = O.sweep_ordered(W, res.Hinv.cpu().numpy(), np.diag(H) == 0, perm, gs, False, True)
    got, base, want = R.proxy_loss(Wz, Qg, H), R.proxy_loss(Wz, rtn, H), R.proxy_loss(Wz, ref["Q"], H)
    print(f"gs {gs}: proxy loss {got:.6f} = {got / base:.4f} x round-to-nearest; CPU restatement on the same factor {want:.6f}, relative "
          f"difference {abs(got - want) / want:.3e} (allowed {10 * LOSS_SPREAD[gs]:.3e}); codes that differ {int((Qg != ref['Q']).sum())}")
    # act-order against natural order under the same (static, or per-channel) scales: printed, not asserted
    plain = gptq_quantize_ordered(Wd, Hd, gs, act_order=False, trace=True) if grouped else gptq_quantize(Wd, Hd, gs, trace=True)
    assert torch.equal(plain.scales.view(torch.int32), res.scales.view(torch.int32)) and plain.perm is None
    natural = R.proxy_loss(Wz, torch.cat([b.Q1 for b in plain.trace], dim=1).cpu().numpy(), H)
    print(f"gs {gs}: proxy loss with act-order {got:.6f}, without it under the same scales {natural:.6f}: ratio {got / natural:.4f}")
    assert got < base
    assert abs(got - want) <= 10 * LOSS_SPREAD[gs] * want


def test_static_groups_without_act_order(trace_input):
    from qqq_amd.quant import gptq_quantize, gptq_quantize_ordered

    W, H = trace_input
    dev = torch.device("cuda:0")
    Wd, Hd = torch.from_numpy(W).to(dev), torch.from_numpy(H).to(dev)
    res = gptq_quantize_ordered(Wd, Hd, 128, act_order=False, static_groups=True, trace=True)
    assert res.perm is None
    _check_trace(res, W, H, np.arange(TRACE_K), True)
    # per-channel static groups have no effect, and with neither switch the flow is gptq_quantize
    for gs, kw in ((-1, dict(act_order=False, static_groups=True)), (-1, dict(act_order=False, static_groups=False)),
                   (128, dict(act_order=False, static_groups=False))):
        assert _same_result(gptq_quantize_ordered(Wd, Hd, gs, **kw), gptq_quantize(Wd, Hd, gs)), (gs, kw)
    with pytest.raises(NotImplementedError, match="gptq_quantize"):  # the plain entry still refuses the switches
        gptq_quantize(Wd, Hd, 128, act_order=True, static_groups=True)


def test_ordered_result_packs_into_a_quantlinear(trace_input):
    from qqq_amd import QuantLinear, pack
    from qqq_amd.quant import gptq_quantize_ordered

    W, H = trace_input
    dev = torch.device("cuda:0")
    for gs in (-1, 128):
        res = gptq_quantize_ordered(torch.from_numpy(W[:64]).to(dev), torch.from_numpy(H).to(dev), gs)
        ql = res.pack_into(QuantLinear(4, gs, TRACE_K, 64, bias=False).to(dev))
        codes = pack.unpack_codes(ql.B, gs != -1).t()  # [N, K]
        assert torch.equal(codes.to(torch.int8), res.codes())
        lo, hi = (0, 15) if gs != -1 else (-7, 7)
        assert int(codes.min()) >= lo and int(codes.max()) <= hi and res.perm is not None


@pytest.mark.parametrize("gs", [-1, 128])
def test_quantize_model_with_act_order_and_static_groups(dev, gs):
    """the reference's default GPTQ switches over the 2-layer model of tests/test_gpu_gptq_model.py: every packed linear holds its
    result's codes, every result carries its order, every linear's proxy loss under its own Hessian is below round-to-nearest under the
    same scales, and the model runs"""
    from test_gpu_gptq_model import CONFIG, LAYERS, LINEARS, _quant_hidden, make_state_dict

    from qqq_amd import pack
    from qqq_amd.quant import FloatDecoderLayer, Hessian, quantize_model, round_to_nearest
    from qqq_amd.quant.model import HESSIAN_OF, _run

    sd, ids = make_state_dict()
    cfg = SimpleNamespace(**CONFIG)
    results = {}
    lm = quantize_model(sd, cfg, ids, gs, device=dev, results=results, act_order=True, static_groups=True)
    assert sorted(results) == sorted(f"model.layers.{i}.{n}" for i in range(LAYERS) for n in LINEARS)
    mods = dict(lm.named_modules())
    for name, res in results.items():
        K = res.weight.shape[1]
        assert res.perm is not None and sorted(res.perm.tolist()) == list(range(K)), name
        assert res.scales.shape[1] == (K // 128 if gs != -1 else 1)
        assert torch.equal(pack.unpack_codes(mods[name].B, gs != -1).t().to(torch.int8), res.codes()), name
    # the Hessians again, as the flow accumulates them: float weights within a layer, quantised layers before it
    inps = torch.nn.functional.embedding(ids.to(dev), sd["model.embed_tokens.weight"].to(dev))
    for i in range(LAYERS):
        prefix = f"model.layers.{i}."
        w = {k[len(prefix):]: v.to(dev) for k, v in sd.items() if k.startswith(prefix)}
        hs = {"qkv": Hessian(256, dev), "o": Hessian(256, dev), "gate_up": Hessian(256, dev), "down": Hessian(512, dev)}
        layer = FloatDecoderLayer(cfg, w)
        _run(layer, inps, 1, {k: h.add_batch for k, h in hs.items()})
        for n in LINEARS:
            res, H = results[prefix + n], hs[HESSIAN_OF[n.split(".")[1]]].H.double()
            Wf = w[n + ".weight"].double()
            Wf[:, torch.diag(H) == 0] = 0
            rtn = round_to_nearest(Wf.half(), res.scales, gs != -1).weight.double()
            loss = lambda Q: float(torch.einsum("ik,kl,il->", Wf - Q, H, Wf - Q))
            got, base = loss(res.weight.double()), loss(rtn)
            print(f"gs {gs} {prefix + n}: proxy loss {got:.4f} = {got / base:.4f} x round-to-nearest")
            assert got < base, prefix + n
            w[n + ".weight"] = res.weight
        inps = _run(layer, inps, 1)
    assert torch.isfinite(_quant_hidden(lm, ids, dev).float()).all()
    toks = lm.generate([ids[0, :5].tolist(), ids[1, :17].tolist()], 4)
    assert all(len(t) == 4 and all(0 <= x < CONFIG["vocab_size"] for x in t) for t in toks)
