"""tests/quant_ref.py on the CPU: the enumeration of the quantiser's exact ties is recomputed and pinned, the kernels' gate is shown to
cover every tie at which the multiply-by-reciprocal is wrong, and the four restatements of the contract (quant_rows_exact,
act_ref.quant_rows, kv8_ref.quant_rows, the C oracle in "recip" mode) are held against each other on the rows built from the ties.
These are facts of IEEE arithmetic; tests/test_gpu_quant_ties.py holds the kernels to them."""
import numpy as np
import pytest
import torch

import act_ref as A
import kv8_ref as K8
import quant_ref as Q

F16, F32, F64 = np.float16, np.float32, np.float64


def test_enumeration_counts():
    t = Q.hard_ties()
    assert len(t.scales) == 24400 and float(t.scales.max()) == 516.0 and float(t.scales.min()) == Q.UNIT
    assert len(t.x) == 83110 and int(np.bincount(t.scale_idx).max()) == 159
    assert int(t.hard.sum()) == 3824 and len(np.unique(t.scale_idx[t.hard])) == 880
    # every tie at which the shortcut is wrong takes the exact division: none is missed by the 0.4995 gate
    assert int((t.hard & ~t.flagged).sum()) == 0
    s_of_tie = t.scales[t.scale_idx]
    sub = s_of_tie < 2.0 ** -14
    assert int((t.hard & sub).sum()) == 673
    binade, count = np.unique(np.floor(np.log2(s_of_tie[t.hard & ~sub].astype(F64))), return_counts=True)
    assert binade.tolist() == list(range(-14, 9)) and set(count.tolist()) == {137}  # 512 ... 516, the last scales, have none
    # the ends of the scale range
    ratio = t.amax_hi.astype(F64) / t.scales
    assert float(ratio.max()) == 190.0 and int(ratio.argmax()) == 0  # at s = 2^-24: the clamp to 127 / -128 happens in legitimate rows
    assert float(t.zero_amax) == 63 * Q.UNIT and float(t.amax_lo[0]) == 64 * Q.UNIT
    # a tie's product is within the gate's reach, and the ties are what the names say
    assert np.array_equal(2.0 * t.x.astype(F64), (2.0 * t.n + 1.0) * s_of_tie.astype(F64))
    assert np.array_equal(Q.scale_of(t.amax_hi), t.scales) and np.array_equal(Q.scale_of(t.amax_lo), t.scales)


def test_the_exact_division_is_round_half_even_everywhere():
    """rint(f32(x / s)) against the exact rounding at the fp16 values on both sides of every half-integer of every reachable scale; both
    are monotone in x, so agreement there is agreement at every reachable (scale, x)."""
    s, x = Q.brackets()
    assert len(x) > 9_000_000
    x64, s64 = x.astype(F64), s.astype(F64)
    n = np.floor(x64 / s64)
    odd = (2.0 * n + 1.0) * s64
    want = np.where(2.0 * x64 == odd, n + np.mod(n, 2.0), n + (2.0 * x64 > odd))
    got = np.rint(x.astype(F32) / s)
    assert got.dtype == F32 and np.array_equal(got.astype(F64), want)
    # ... and the shortcut with its gate as well; without the gate it is wrong at the hard ties and only there
    p = x.astype(F32) * (F32(1) / s)
    q = np.rint(p)
    assert np.array_equal(np.where(np.abs(p - q) > Q.GATE, got, q).astype(F64), want)
    wrong = q.astype(F64) != want
    t = Q.hard_ties()
    keys = lambda sc, xv: np.unique((sc.astype(F16).view(np.uint16).astype(np.uint32) << 16) | xv.view(np.uint16))
    assert np.array_equal(keys(s[wrong], x[wrong]), keys(t.scales[t.scale_idx[t.hard]], t.x[t.hard]))


@pytest.mark.parametrize("L", [8, 64, 128, 1024])
def test_corpus_holds_every_hard_tie(L):
    t = Q.hard_ties()
    c = Q.corpus(L)
    assert c.rows.dtype == F16 and c.rows.shape[1] == L and np.isfinite(c.rows).all()
    # every row has the scale it was built for, from an amax that appears in both signs
    assert np.array_equal(Q.scale_of(np.abs(c.rows).max(1)), t.scales[c.scale_idx])
    assert np.array_equal(c.rows.max(1), t.amax_hi[c.scale_idx]) and np.array_equal(c.rows.min(1), -t.amax_hi[c.scale_idx])
    assert len(np.unique(c.scale_idx)) == 880
    sb = t.scales[t.scale_idx[t.hard]].astype(F16).view(np.uint16).astype(np.uint32) << 16
    xb = t.x[t.hard].view(np.uint16).astype(np.uint32)
    want = np.unique(np.concatenate([sb | xb, sb | xb | 0x8000]))  # both signs
    assert len(want) == 2 * 3824 and np.array_equal(Q.hard_tie_keys(c.rows), want)
    # the amax reaches every element index
    assert len(np.unique(c.rows.argmax(1))) == min(L, len(c.rows))
    if L >= 128:  # room for the filler
        assert (c.rows == 0).any() and np.signbit(c.rows[c.rows == 0]).any() and not np.signbit(c.rows[c.rows == 0]).all()


def _rows_under_test():
    return [np.concatenate([Q.corpus(L).rows, Q.edge_rows(L)]) for L in (8, 64, 128, 1024)]


def test_the_four_restatements_agree_on_the_corpus():
    from oracle import c_oracle as C

    for y in _rows_under_test():
        q, s1 = Q.quant_rows_exact(y)
        live = s1[:, 0] > 0
        assert int((~live).sum()) == 3  # the two all-zero rows and the row whose amax is 63 * 2^-24
        assert not q[~live].any()
        assert np.array_equal(Q.shortcut_codes(y), q)
        if y.shape[1] == 8:
            assert int((Q.shortcut_codes(y, None) != q).sum()) == 2 * 3824  # without the fallback: wrong at every hard tie
        aq, as1 = A.quant_rows(y)
        assert np.array_equal(as1.view(np.uint32), s1.view(np.uint32)) and np.array_equal(aq[live], q[live])
        assert not aq[~live].any()
        kq, ks = K8.quant_rows(torch.from_numpy(y))
        assert np.array_equal(ks.numpy().view(np.uint32), s1[:, 0].view(np.uint32)) and np.array_equal(kq.numpy(), q)
        oq, os1 = C.dynamic_quant(y[live], "recip")
        assert np.array_equal(os1.view(np.uint32), s1[live].view(np.uint32)) and np.array_equal(oq, q[live])


def test_edge_rows_quantise_as_documented():
    for L in (8, 64, 4096):
        y = Q.edge_rows(L)
        q, s1 = Q.quant_rows_exact(y)
        assert s1[:3, 0].tolist() == [0.0, 0.0, 0.0] and not q[:3].any() and np.abs(y[2]).max() == F16(63 * Q.UNIT)
        assert float(s1[3, 0]) == Q.UNIT and np.array_equal(q[3].astype(F64) * Q.UNIT, y[3].astype(F64))  # every element is its own code
        assert float(s1[4, 0]) == Q.UNIT
        units = np.rint(y[4].astype(F64) / Q.UNIT)
        assert {190.0, -190.0, 129.0, -129.0, 128.0, -128.0, 127.0, -127.0} <= set(units.tolist())
        assert np.array_equal(q[4], np.clip(units, -128, 127).astype(np.int8)) and q[4].min() == -128 and q[4].max() == 127
        assert float(s1[5, 0]) == 516.0 and q[5].max() == 127 and q[5].min() == -127  # 65504 / 516 = 126.9
        assert np.count_nonzero(y[6]) == 1 and y[6, -1] != 0 and q[6, -1] == -127 and not q[6, :-1].any()
