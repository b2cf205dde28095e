"""ops.token_logprobs on the GPU against tests/score_ref.py (float64 numpy): values within a derived tolerance, the argmax against the
sampler at temperature 0, bit-for-bit reproducibility (row index, ld, permutation, graph replay), and the special values.

The tolerance, derived and not measured.  The kernel forms each weight's exponent a = (l - l_max) * log2 e in f32 from three roundings (the
difference, the constant, the product); |a| <= 44 matters, below that the weight truncates to 0.  An error of 44 * 3 * 2^-24 in the exponent
is a relative error of 44 * 3 * 2^-24 * ln 2 ~ 5.5e-6 in the weight, hence at most that in W (all weights are non-negative).  exp2f adds
about 2 * 2^-23 ~ 2.4e-7, the truncation to multiples of 2^-44 at most 2^18 * 2^-44 ~ 1.5e-8 of a W >= 1.  ln W inherits the relative error
of W: 5.8e-6 together, below 8e-6.  The difference l_t - l_max and the logarithm are in f64; the result is rounded to f32 once:
2^-24 |ref| for a normal result, 2^-23 |ref| allowed.  Together  |got - ref| <= 8e-6 + 2^-23 |ref|.
A float32 emulation of this arithmetic on the CPU used at most 0.24 of the bound (random rows of up to 262 144 entries, scales 0.5 to 30)."""
import numpy as np
import pytest
import torch

from score_ref import token_logprobs as ref_logprobs, tolerance

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8), (7, 8), (63, 64), (64, 64), (65, 72), (1001, 1008), (32000, 32000), (65537, 65544), (151936, 151936)]
SCALES = (1.0, 30.0, 0.5, 4.0, 10.0)  # row r is scaled by SCALES[r % 5]; 30 pushes most weights below 2^-44


def _padded(logits: np.ndarray, ld: int, dev, fill=65504.0):
    """the rows as a [rows, vocab] view of an fp16 [rows, ld] device matrix whose padding columns hold `fill`"""
    rows, vocab = logits.shape
    buf = torch.full((rows, ld), fill, dtype=torch.float16, device=dev)
    buf[:, :vocab] = torch.from_numpy(logits).to(dev)
    return buf[:, :vocab]


def _run(logits, targets, return_argmax=True):
    from qqq_amd import ops

    t = torch.as_tensor(np.asarray(targets, dtype=np.int64)).to(logits.device)
    lp, am = ops.token_logprobs(logits, t, return_argmax)
    torch.cuda.synchronize()
    assert lp.dtype == torch.float32 and lp.shape == (logits.shape[0],)
    if not return_argmax:
        assert am is None
        return lp.cpu().numpy(), None
    assert am.dtype == torch.int64 and am.shape == (logits.shape[0],)
    return lp.cpu().numpy(), am.cpu().numpy()


def _rows(vocab, rows, seed):
    rng = np.random.default_rng(seed)
    l = rng.standard_normal((rows, vocab))
    for r in range(rows):
        l[r] *= SCALES[r % len(SCALES)]
    return l.astype(np.float16)


def _close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{what}: max |got - ref| = {err.max():.3e}, max share of the bound = {(err / tolerance(ref)).max():.3f}")
    assert (err <= tolerance(ref)).all(), (what, got, ref)


# ---- 1. values

@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_values_against_the_float64_reference(dev, vocab, ld, rows):
    l = _rows(vocab, rows, vocab * 11 + rows)
    x = _padded(l, ld, dev)  # the padding columns hold 65504: they must not win and must not be summed
    f = l.astype(np.float64)
    for place, t in (("first", np.zeros(rows, np.int64)), ("last", np.full(rows, vocab - 1)), ("max", f.argmax(1)), ("min", f.argmin(1))):
        ref, ref_am = ref_logprobs(l, t)
        got, am = _run(x, t)
        _close(got, ref, f"vocab {vocab} ld {ld} rows {rows} target {place}")
        assert am.tolist() == ref_am.tolist() == f.argmax(1).tolist()
        assert np.isfinite(got).all()
        lp_only, _ = _run(x, t, return_argmax=False)
        assert np.array_equal(lp_only.view(np.uint32), got.view(np.uint32))


def test_a_target_far_below_the_maximum_keeps_its_log_probability(dev):
    """Rows scaled by 30: most weights, the target's among them, truncate to 0.  The result is still (l_t - l_max) - ln W."""
    vocab = 32000
    l = (30.0 * np.random.default_rng(5).standard_normal((4, vocab))).astype(np.float16)
    f = l.astype(np.float64)
    t = f.argmin(1)
    assert ((f[np.arange(4), t] - f.max(1)) * np.log2(np.e) < -60).all()  # far below 2^-44
    ref, _ = ref_logprobs(l, t)
    W = np.exp(f - f.max(1, keepdims=True)).sum(1)
    assert np.allclose(ref, f[np.arange(4), t] - f.max(1) - np.log(W), rtol=1e-14, atol=0)
    got, _ = _run(torch.from_numpy(l).to(dev), t)
    _close(got, ref, "far-below targets")
    assert (got < -100).all()


# ---- 2. argmax is the sampler's greedy token

@pytest.mark.parametrize("vocab,ld", [(7, 8), (65, 72), (1001, 1008), (32000, 32000), (151936, 151936)])
def test_argmax_equals_sample_tokens_at_temperature_0(dev, vocab, ld):
    from qqq_amd import ops

    rng = np.random.default_rng(vocab)
    rows = 6
    l = rng.standard_normal((rows, vocab)).astype(np.float16)
    l[0, 0] = 30.0                                    # the maximum at the first entry
    l[1, vocab - 1] = 30.0                            # ... at the last
    ties = sorted(rng.choice(vocab, size=3, replace=False).tolist())
    l[2, ties] = 30.0                                 # a tie: the lowest index
    l[3, [0, vocab - 1]] = 30.0                       # a tie between both ends
    l[4, :] = -2.5                                    # everything ties
    x = _padded(l, ld, dev)
    _, am = _run(x, np.zeros(rows, np.int64))
    greedy = ops.sample_tokens(x, 0.0, 0, 1.0, torch.zeros(rows, device=dev))
    torch.cuda.synchronize()
    assert am.tolist() == greedy.tolist() == l.astype(np.float64).argmax(1).tolist()
    assert am[:5].tolist() == [0, vocab - 1, ties[0], 0, 0]


# ---- 3. reproducibility, bit for bit

def test_same_row_same_bits_wherever_it_sits_and_however_it_is_ordered(dev):
    vocab = 40003  # 40 full rounds of 1024 lanes minus a bit, and a tail of 3
    rng = np.random.default_rng(77)
    row = (6.0 * rng.standard_normal(vocab)).astype(np.float16)
    t = int(rng.integers(vocab))
    other = rng.standard_normal((5, vocab)).astype(np.float16)
    a = other.copy()
    a[0], a[3] = row, row
    got_a, am_a = _run(_padded(a, vocab + 5, dev), [t, 1, 2, t, 4])
    b = other[:3].copy()
    b[2] = row
    got_b, am_b = _run(_padded(b, vocab + 5 + 8 * 37, dev), [0, 1, t])
    got_c, am_c = _run(torch.from_numpy(row[None].copy()).to(dev), [t])  # an unpadded view: the op copies it into padded rows
    bits = {int(v.view(np.uint32)) for v in (got_a[0], got_a[3], got_b[2], got_c[0])}
    assert len(bits) == 1 and am_a[0] == am_a[3] == am_b[2] == am_c[0]
    # a permutation of the row with the target moved along: the integer sum does not depend on the order
    perm = rng.permutation(vocab)
    shuffled = row[perm]
    got_p, _ = _run(torch.from_numpy(np.stack([shuffled, row])).to(dev), [int(np.nonzero(perm == t)[0][0]), t])
    assert int(got_p[0].view(np.uint32)) == int(got_p[1].view(np.uint32)) == bits.pop()
    ref, _ = ref_logprobs(row[None], [t])
    _close(got_p[1:], ref, "the repeated row")


def test_hipgraph_replays_with_everything_updated_in_place(dev):
    from qqq_amd import ops

    rows, vocab = 6, 4099
    g = torch.Generator(device=dev).manual_seed(1)
    buf = torch.zeros((rows, vocab + 5), dtype=torch.float16, device=dev)
    logits = buf[:, :vocab]
    targets = torch.zeros(rows, dtype=torch.int64, device=dev)

    def fill(i):
        logits.copy_((3.0 * torch.randn((rows, vocab), generator=g, device=dev)).half())
        targets.copy_(torch.randint(0, vocab, (rows,), generator=g, device=dev))
        targets[i % rows] = -1

    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.token_logprobs(logits, targets)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            lp, am = ops.token_logprobs(logits, targets)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for i in range(1, 4):
        fill(i)
        graph.replay()
        torch.cuda.synchronize()
        want_lp, want_am = ops.token_logprobs(logits, targets)
        torch.cuda.synchronize()
        assert torch.equal(lp.view(torch.int32), want_lp.view(torch.int32)) and torch.equal(am, want_am)
        ref, ref_am = ref_logprobs(logits.cpu().numpy(), targets.cpu().numpy())
        _close(lp.cpu().numpy(), ref, f"replay {i}")
        assert am.tolist() == ref_am.tolist() and float(lp[i % rows]) == 0.0
        seen.append(lp.tolist())
    assert seen[0] != seen[1] and seen[1] != seen[2]  # the replays read the new contents


# ---- 4. the special values, one assertion each

def test_special_values(dev):
    vocab, ld = 300, 304
    rng = np.random.default_rng(3)
    base = rng.standard_normal(vocab).astype(np.float16)
    base[17] = 5.0  # the maximum of the plain rows
    rows, targets = [], []

    def add(row, t):
        rows.append(row)
        targets.append(t)
        return len(rows) - 1

    ign1 = add(base.copy(), -1)
    ign100 = add(base.copy(), -100)
    oob = add(base.copy(), vocab)          # the first padding column: outside
    oob_far = add(base.copy(), 1 << 40)
    a = base.copy(); a[40] = np.nan; nan_t = add(a, 40)
    a = base.copy(); a[41] = -np.inf; ninf_t = add(a, 41)
    a = base.copy(); a[::2] = np.nan; a[1] = -np.inf; holes = add(a, 17)          # NaN and -inf beside the target have no weight
    a = base.copy(); a[[7, 200, 250]] = np.inf; inf_in = add(a, 200)              # +inf maxima: a target in the group
    inf_out = add(a.copy(), 17)                                                   # ... and a finite target
    empty_ninf = add(np.full(vocab, -np.inf, np.float16), 5)                      # no logit above -inf
    empty_nan = add(np.full(vocab, np.nan, np.float16), 5)
    empty_ign = add(np.full(vocab, np.nan, np.float16), -1)
    a = np.full(vocab, -np.inf, np.float16); a[[10, 20]] = [-0.0, 0.0]; zeros = add(a, 20)  # -0 ties with +0
    l = np.stack(rows)
    got, am = _run(_padded(l, ld, dev, fill=float("inf")), targets)
    ref, ref_am = ref_logprobs(l, targets)
    assert got[ign1] == 0.0 and not np.signbit(got[ign1])
    assert got[ign100] == 0.0
    assert np.isnan(got[oob])
    assert np.isnan(got[oob_far])
    assert got[nan_t] == -np.inf
    assert got[ninf_t] == -np.inf
    assert abs(got[holes] - ref[holes]) <= tolerance(ref[holes]) and np.isfinite(got[holes])
    assert abs(got[inf_in] + np.log(3.0)) <= tolerance(np.log(3.0)) and am[inf_in] == 7
    assert got[inf_out] == -np.inf
    assert np.isnan(got[empty_ninf]) and am[empty_ninf] == 0
    assert np.isnan(got[empty_nan]) and am[empty_nan] == 0
    assert got[empty_ign] == 0.0 and am[empty_ign] == 0
    assert abs(got[zeros] + np.log(2.0)) <= tolerance(np.log(2.0)) and am[zeros] == 10
    assert am.tolist() == ref_am.tolist()
    # whatever the target, the argmax of a plain row is untouched
    assert am[ign1] == am[oob] == am[nan_t] == 17
    # every entry agrees with the reference's class: NaN, -inf, 0 or within the tolerance
    for r in range(len(rows)):
        if np.isnan(ref[r]):
            assert np.isnan(got[r]), r
        elif np.isinf(ref[r]):
            assert got[r] == ref[r], r
        else:
            assert abs(got[r] - ref[r]) <= tolerance(ref[r]), r


def test_shape_dtype_and_device_errors_raise_before_any_launch(dev):
    from qqq_amd import ops

    logits = torch.zeros((3, 40), dtype=torch.float16, device=dev)
    t = torch.zeros(3, dtype=torch.int64, device=dev)
    for bad_logits, bad_t in ((logits.float(), t), (logits, t.int()), (logits, t[:2]), (logits, t.cpu()), (logits.cpu(), t), (logits[0], t),
                              (logits[:, :0], t)):
        with pytest.raises(RuntimeError, match="token_logprobs: "):
            ops.token_logprobs(bad_logits, bad_t)
    lp, am = ops.token_logprobs(logits[:0], t[:0])
    assert lp.shape == (0,) and am.shape == (0,)
