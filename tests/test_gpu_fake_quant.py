"""ops.fake_quant_rows on the GPU, bit for bit on uint16 views against the numpy restatement (tests/smooth_ref.py, itself held to the
reference's recorded operands by tests/test_smooth_ref_cpu.py): every width at which the kernel takes another path (one workgroup per row
with 1, 2, 4 or 8 units of 8 columns per thread in registers up to 16384 columns, the re-read walk above; one unit per thread with the
reduction inside 16 lanes for groups of 128), rows 1 / 3 / 65, both operand sides and bit widths, views, in place, crafted rows, graph
replay, a row offset past 2^31 elements, and every refusal."""
import numpy as np
import pytest
import torch

import smooth_ref as R

pytestmark = pytest.mark.gpu

ROW_COLS = (8, 136, 2056, 8192, 11008, 16392, 24576)  # 1, 1, 2 (one past 2048), 4, 8, and two widths of the re-read walk
GROUP_COLS = (128, 384, 2176)
ROWS = (1, 3, 65)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _same(a, b):
    return a.dtype == b.dtype == np.float16 and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _matrix(seed, rows, cols):
    """random rows with a few outlier columns; where there is room: an all-zero row, a row at 1e-6 (the eps clamp), a one-sided row"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, cols)) * 2.5
    x[:, rng.integers(0, cols, 3)] *= 20
    x = x.astype(np.float16)
    if rows >= 3:
        x[1] = 0
        x[2] = (rng.standard_normal(cols) * 1e-6).astype(np.float16)
    if rows >= 65:
        x[7] = -np.abs(x[7])
        x[8] = np.abs(x[8])
        x[9] = (rng.standard_normal(cols) * 3e-8).astype(np.float16)  # subnormals below the eps scale
    return x


def _scale(seed, cols):
    rng = np.random.default_rng(seed + 1000)
    return np.where(rng.random(cols) < 0.3, rng.random(cols) * 7 + 1, 1).astype(np.float16)  # mixed 1 and > 1


def _check(dev, x, group):
    from qqq_amd.quant import ops

    cols = x.shape[1]
    c = _scale(cols, cols)
    xd, cd = torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev)
    for bits in (8, 4):
        for divide in (True, False):
            for cs, csd in ((None, None), (c, cd)):
                got = ops.fake_quant_rows(xd, csd, bits, group, divide).cpu().numpy()
                ref = R.fake_quant_rows(x, cs, bits, group, divide)
                assert _same(got, ref), (x.shape, group, bits, divide, cs is None, int((_bits(got) != _bits(ref)).sum()))
                assert not (_bits(got) == 0x8000).any()  # no -0
    assert torch.equal(xd.cpu(), torch.from_numpy(x))  # x is left as it is


@pytest.mark.parametrize("cols", ROW_COLS)
def test_per_row_has_the_restatements_bits(dev, cols):
    for rows in ROWS:
        _check(dev, _matrix(cols + rows, rows, cols), 0)


@pytest.mark.parametrize("cols", GROUP_COLS)
def test_per_group_has_the_restatements_bits(dev, cols):
    for rows in ROWS:
        _check(dev, _matrix(cols + rows, rows, cols), 128)


def test_crafted_rows(dev):
    """an all-zero row gives zeros under the eps scale; a row at 1e-6 is clamped by it; exact .5 ties go to even; no -0 anywhere"""
    from qqq_amd.quant import ops

    x = np.zeros((4, 136), np.float16)
    x[1, :8] = [127, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5]  # scale exactly 1 at 8 bits
    x[2, :8] = [7, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, -7]  # ... and at 4 bits
    x[3] = np.float16(1e-6)
    x[3, ::2] *= -1
    xd = torch.from_numpy(x).to(dev)
    y8 = ops.fake_quant_rows(xd, None, 8).cpu().numpy()
    y4 = ops.fake_quant_rows(xd, None, 4).cpu().numpy()
    assert y8[1, :8].tolist() == [127, 0, 2, 2, 0, -2, -2, 4] and y4[2, :8].tolist() == [7, 0, 2, 2, 0, -2, -2, -7]
    assert not y8[0].any() and not y4[0].any()
    for y, bits in ((y8, 8), (y4, 4)):
        assert _same(y, R.fake_quant_rows(x, None, bits)) and not (_bits(y) == 0x8000).any()
    # 1e-6 is 17 fp16 subnormal steps; 17 / 127 rounds below the eps 2^-23, so the scale is the eps and the codes are +-8 or 9
    eps = np.float16(1.1920929e-07)
    codes = y8[3].astype(np.float64) / float(eps)
    assert np.array_equal(codes, np.rint(codes)) and np.abs(codes).max() <= 127 and np.abs(codes).min() >= 1
    # the weight side: a column scale > 1 on the negative tie flips nothing to -0
    c = np.ones(136, np.float16)
    c[4] = 3
    y = ops.fake_quant_rows(xd, torch.from_numpy(c).to(dev), 8, 0, True).cpu().numpy()
    assert _same(y, R.fake_quant_rows(x, c, 8, 0, True)) and not (_bits(y) == 0x8000).any()


def test_views_in_place_and_given_outputs(dev):
    from qqq_amd.quant import ops

    rows, cols = 5, 2056
    x = _matrix(5, rows, cols)
    c = _scale(5, cols)
    cd = torch.from_numpy(c).to(dev)
    for group, lo, hi in ((0, 8, 8 + cols), (128, 128, 128 + 1920)):
        wide = torch.zeros((rows, cols + 264), dtype=torch.float16, device=dev)
        wide[:, 8:8 + cols] = torch.from_numpy(x).to(dev)
        view = wide[:, lo:hi]  # a strided view: row stride 2320, base 16-byte aligned
        xs, cs, csd = x[:, lo - 8:hi - 8], c[lo - 8:hi - 8].copy(), cd[lo - 8:hi - 8].clone()
        ref = R.fake_quant_rows(xs, cs, 4, group, False)
        assert _same(ops.fake_quant_rows(view, csd, 4, group, False).cpu().numpy(), ref)
        out_wide = torch.full((rows, cols + 16), 9.0, dtype=torch.float16, device=dev)
        out = out_wide[:, 8:8 + hi - lo]
        assert ops.fake_quant_rows(view, csd, 4, group, False, out=out) is out
        assert _same(out.cpu().numpy(), ref) and bool((out_wide[:, :8] == 9).all()) and bool((out_wide[:, 8 + hi - lo:] == 9).all())
        before = wide.clone()
        assert ops.fake_quant_rows(view, csd, 4, group, False, out=view) is view  # in place
        assert _same(view.cpu().numpy(), ref)
        before[:, lo:hi] = view
        assert torch.equal(wide, before)  # nothing outside the view moved
    # in place on the re-read walk too
    x = _matrix(6, 3, 16392)
    xd = torch.from_numpy(x).to(dev)
    ops.fake_quant_rows(xd, None, 8, out=xd)
    assert _same(xd.cpu().numpy(), R.fake_quant_rows(x, None, 8))


def test_a_row_offset_past_2_to_the_31(dev):
    """rows 2^30 + 8 elements apart: the third row starts past element 2^31 of its buffer; the rows between are never touched"""
    from qqq_amd.quant import ops

    cols, ld = 384, 2 ** 30 + 8
    x = _matrix(31, 3, cols)
    for group in (0, 128):
        buf = torch.empty(2 * ld + cols, dtype=torch.float16, device=dev)
        view = buf.as_strided((3, cols), (ld, 1))
        view.copy_(torch.from_numpy(x).to(dev))
        out = ops.fake_quant_rows(view, None, 8, group)
        assert _same(out.cpu().numpy(), R.fake_quant_rows(x, None, 8, group))
        ops.fake_quant_rows(view, None, 8, group, out=view)
        assert _same(view.cpu().numpy(), R.fake_quant_rows(x, None, 8, group))
        del buf, view


def test_replays_from_a_captured_graph(dev):
    from qqq_amd.quant import ops

    rows, cols = 5, 2176
    X = torch.zeros((rows, cols), dtype=torch.float16, device=dev)
    C = torch.ones(cols, dtype=torch.float16, device=dev)
    Yr, Yg = torch.zeros_like(X), torch.zeros_like(X)
    ops.fake_quant_rows(X, C, 8, 0, True, out=Yr)  # warm-up outside the capture
    ops.fake_quant_rows(X, C, 4, 128, False, out=Yg)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.fake_quant_rows(X, C, 8, 0, True, out=Yr)
        ops.fake_quant_rows(X, C, 4, 128, False, out=Yg)
    for seed in (1, 2):
        x, c = _matrix(seed, rows, cols), _scale(seed, cols)
        X.copy_(torch.from_numpy(x))
        C.copy_(torch.from_numpy(c))
        Yr.zero_()
        Yg.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert _same(Yr.cpu().numpy(), R.fake_quant_rows(x, c, 8, 0, True)) and _same(Yg.cpu().numpy(), R.fake_quant_rows(x, c, 4, 128, False))
        assert torch.equal(Yr, ops.fake_quant_rows(X, C, 8, 0, True)) and torch.equal(Yg, ops.fake_quant_rows(X, C, 4, 128, False))  # eager


def test_every_argument_rejection(dev):
    from qqq_amd.quant import ops

    x = torch.zeros((4, 256), dtype=torch.float16, device=dev)
    c = torch.ones(256, dtype=torch.float16, device=dev)
    f = ops.fake_quant_rows
    bad = [
        (lambda: f(x.float(), c, 8), "fake_quant_rows: x must be a float16 matrix"),
        (lambda: f(x[0], c, 8), "fake_quant_rows: x must be a float16 matrix"),
        (lambda: f(x[:, :12], None, 8), "fake_quant_rows: x has the shape"),
        (lambda: f(torch.zeros((256, 8), dtype=torch.float16, device=dev).t(), None, 8), "fake_quant_rows: x must have unit column stride"),
        (lambda: f(torch.zeros((4, 260), dtype=torch.float16, device=dev)[:, :256], c, 8), "a multiple of 8, got strides"),
        (lambda: f(x[:, 4:12], None, 8), "fake_quant_rows: x must be 16-byte aligned"),
        (lambda: f(x, c, 6), "fake_quant_rows: bits must be 8 or 4"),
        (lambda: f(x, c, 8, group=64), "fake_quant_rows: group must be 0"),
        (lambda: f(x[:, :136], None, 8, group=128), "no multiple of group = 128"),
        (lambda: f(x, c[:128], 8), r"col_scale must be None or contiguous float16 \[256\]"),
        (lambda: f(x, c.float(), 8), "col_scale must be None or contiguous float16"),
        (lambda: f(x, torch.ones(512, dtype=torch.float16, device=dev)[::2], 8), "col_scale must be None or contiguous float16"),
        (lambda: f(x, torch.ones(264, dtype=torch.float16, device=dev)[4:260], 8), "col_scale must be 16-byte aligned"),
        (lambda: f(x, c, 8, out=torch.zeros((4, 128), dtype=torch.float16, device=dev)), "fake_quant_rows: out has the shape"),
        (lambda: f(x, c, 8, out=torch.zeros((4, 256), dtype=torch.float32, device=dev)), "fake_quant_rows: out must be a float16 matrix"),
        (lambda: f(x, c.cpu(), 8), "every tensor must be on the GPU"),
        (lambda: f(x.cpu(), None, 8), "every tensor must be on the GPU"),
    ]
    for call, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            call()
    wide = torch.zeros((4, 512), dtype=torch.float16, device=dev)
    with pytest.raises(RuntimeError, match="out starts where x does with another row stride"):
        f(wide[:, :256], None, 8, out=wide.view(8, 256)[:4])
    with pytest.raises(RuntimeError, match="qqq_fake_quant_rows: X and Y overlap"):
        f(wide[:, :256], None, 8, out=wide[:, 128:384])
    torch.cuda.synchronize()
    assert not wide.any()  # nothing was launched
