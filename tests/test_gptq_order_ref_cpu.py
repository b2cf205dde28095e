"""GPTQ with act-order and static groups without a GPU: the CPU restatement (tests/gptq_order_ref.py) against the fixture recorded from
the reference's own GPTQ.fasterquant(actorder, static_groups) (tests/golden/gptq_order_small.npz, gen_gptq_order_golden.py), what the
fixture exercises, the binding of the two entries from a header of their own, and the refusals of the entries and the Python layer."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gptq_order_ref as O
import gptq_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = 77
# (group size, act-order, static groups, mse): gen_gptq_order_golden.py's five settings
SETTINGS = [(-1, True, False, False), (-1, True, False, True), (128, True, True, False), (128, True, True, True), (128, False, True, False)]


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "gptq_order_small.npz"))
    K = g["W"].shape[1]
    iu = np.triu_indices(K)
    H = np.zeros((K, K), np.float32)
    H[iu] = g["H_triu"]
    H = H + np.triu(H, 1).T
    factors = {}
    for act, name in ((True, "Hinv_perm_triu"), (False, "Hinv_triu")):
        factors[act] = np.zeros((K, K), np.float32)
        factors[act][iu] = g[name]
    return g, H, factors


@pytest.mark.parametrize("gs,act,static,mse", SETTINGS)
def test_restatement_reproduces_the_reference_bit_for_bit(fixture, gs, act, static, mse):
    g, H, factors = fixture
    tag = f"g{gs}_act{int(act)}_static{int(static)}_mse{int(mse)}"
    r = O.sweep_ordered(g["W"], factors[act], np.diag(H) == 0, g["perm"] if act else None, gs, mse, static)
    assert np.array_equal(r["scales"].view(np.int32), g[tag + "/scales"].view(np.int32))
    assert np.array_equal(R.codes(r["weight"], r["scales"], gs != -1), g[tag + "/codes"])
    assert np.array_equal(r["weight"].view(np.int16), g[tag + "/weight"].view(np.int16))
    if gs != -1:
        assert np.array_equal(r["s_extra"].view(np.int32), g[tag + "/s_extra"].view(np.int32))
        assert r["scales"].shape == (g["W"].shape[0], g["W"].shape[1] // 128)  # natural group order: an ordinary checkpoint
    else:
        assert r["s_extra"] is None and tag + "/s_extra" not in g.files
    lo, hi = (0, 15) if gs != -1 else (-7, 7)
    assert g[tag + "/codes"].min() >= lo and g[tag + "/codes"].max() <= hi
    assert not r["weight"][:, DEAD].any()


def test_fixture_exercises_the_per_column_path_and_the_order_of_the_steps(fixture):
    g, H, _ = fixture
    perm, W = g["perm"], g["W"].astype(np.float32)
    K = W.shape[1]
    assert sorted(perm.tolist()) == list(range(K))
    for i1 in range(0, K, 128):  # every block of the swept order holds columns of both groups
        assert set((perm[i1:i1 + 128] // 128).tolist()) == {0, 1}, i1
    # the dead column holds the row's and its group's maximum in the even rows: the per-channel scale sees it, the group scale does not
    assert np.diag(H)[DEAD] == 0 and (np.diag(H) == 0).sum() == 1
    assert (np.abs(W[::2]).argmax(axis=1) == DEAD).all() and (np.abs(W[1::2, DEAD]) < 0.1).all()
    assert np.array_equal(g["g-1_act1_static0_mse0/scales"][::2, 0], np.full(32, np.float32(W[0, DEAD]) / np.float32(7), np.float32))
    Wz = W.copy()
    Wz[:, DEAD] = 0
    assert np.array_equal(g["g128_act1_static1_mse0/scales"].view(np.int32), O.group_scales(Wz).view(np.int32))
    assert not np.array_equal(g["g128_act1_static1_mse0/scales"][::2, 0], O.group_scales(W)[::2, 0])
    # static groups are the same scales with and without act-order; the codes are not
    assert np.array_equal(g["g128_act1_static1_mse0/scales"], g["g128_act0_static1_mse0/scales"])
    assert (g["g128_act1_static1_mse0/codes"] != g["g128_act0_static1_mse0/codes"]).any()


def test_recorded_perm_is_a_descending_order_of_the_diagonal(fixture):
    g, H, _ = fixture
    d = np.diag(H).copy()
    d[d == 0] = 1  # the dead-column rule
    along = d[g["perm"]]
    assert (along[:-1] >= along[1:]).all()
    # no exactly equal entries here, so the stable order gptq_quantize_ordered takes is the recorded one
    assert len(set(d.tolist())) == d.size and np.array_equal(np.argsort(-d, kind="stable"), g["perm"])
    assert np.array_equal(O.hinv_of_permuted(H)[2], g["perm"])


def test_fixture_factor_is_the_cholesky_chain_of_the_permuted_hessian(fixture):
    g, H, factors = fixture
    again, dead, perm = O.hinv_of_permuted(H, g["perm"])
    assert dead.sum() == 1 and dead[DEAD]
    assert np.allclose(np.triu(again), factors[True], rtol=1e-3, atol=1e-6 * np.abs(factors[True]).max())


def test_block_cols_with_one_scale_per_row_is_block(fixture):
    g, H, factors = fixture
    W = g["W"].astype(np.float32)[:, :128]
    s = R.scales(W, True)
    q0, e0 = R.block(W, factors[True][:128, :128], s, True)
    q1, e1 = O.block_cols(W, factors[True][:128, :128], np.repeat(s[:, None], 128, axis=1))
    assert np.array_equal(q0.view(np.int32), q1.view(np.int32)) and np.array_equal(e0.view(np.int32), e1.view(np.int32))


def test_library_binds_the_two_entries_from_a_header_of_their_own():
    from qqq_amd import _abi, build
    from qqq_amd.quant import _lib as qlib

    L = qlib.lib()
    header, rotate = (os.path.join(build.QUANT_INCLUDE, h) for h in ("qqq_amd_gptq_order.h", "qqq_amd_rotate.h"))
    protos = _abi.prototypes(header)
    assert set(protos) == {"qqq_gptq_group_scales", "qqq_gptq_block_cols"}
    for name, (_, params) in protos.items():
        assert len(getattr(L, name).argtypes or []) == len(params), name
        for p in params:
            assert _abi.ctype_of(p) in (ctypes.c_void_p, ctypes.c_int), p
    assert header in build.quant_headers() and os.path.dirname(header) == os.path.dirname(build.QUANT_HEADER)
    assert not set(protos) & set(_abi.prototypes(build.QUANT_HEADER)) and not set(protos) & set(_abi.prototypes(rotate))
    assert L.qqq_quant_abi_version() == qlib.ABI_VERSION == 1


def _refused(fn, *args):
    from qqq_amd.quant import _lib as qlib

    rc = fn(*args)
    return rc, qlib.last_error()


def test_entries_refuse_bad_arguments_by_name():
    from qqq_amd.quant import _lib as qlib

    L = qlib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok_block = dict(W1=p, ldw=128, Hinv1=p, ldh=128, scales=p, lds=3, groups=3, gidx=p, rows=4, count=128, Q1=p, ldq=128, Err1=p, lde=128)

    def block(**kw):
        a = dict(ok_block, **kw)
        return _refused(L.qqq_gptq_block_cols, a["W1"], a["ldw"], a["Hinv1"], a["ldh"], a["scales"], a["lds"], a["groups"], a["gidx"], a["rows"],
                        a["count"], a["Q1"], a["ldq"], a["Err1"], a["lde"], 0, None)

    for kw in (dict(count=96), dict(count=0), dict(rows=0), dict(groups=0), dict(groups=-1), dict(lds=2), dict(ldw=127), dict(ldh=64),
               dict(ldq=100), dict(lde=1), dict(W1=None), dict(Hinv1=None), dict(scales=None), dict(gidx=None), dict(Q1=None), dict(Err1=None),
               dict(W1=p + 2), dict(scales=p + 1), dict(gidx=p + 2), dict(Err1=p + 1)):
        rc, msg = block(**kw)
        assert rc == qlib.ERR_ARG and msg.startswith("qqq_gptq_block_cols: "), (kw, rc, msg)

    ok_scales = dict(W=p, ldw=256, rows=4, cols=256, mse=0, out=p, lds=2)

    def scales(**kw):
        a = dict(ok_scales, **kw)
        return _refused(L.qqq_gptq_group_scales, a["W"], a["ldw"], a["rows"], a["cols"], a["mse"], a["out"], a["lds"], 0, None)

    for kw in (dict(rows=0), dict(cols=0), dict(cols=192), dict(cols=64, ldw=64), dict(cols=1 << 21, ldw=1 << 21, lds=1 << 14), dict(ldw=128),
               dict(lds=1), dict(mse=3), dict(mse=-1), dict(W=None), dict(out=None), dict(W=p + 1), dict(out=p + 2)):
        rc, msg = scales(**kw)
        assert rc == qlib.ERR_ARG and msg.startswith("qqq_gptq_group_scales: "), (kw, rc, msg)


def test_python_layer_refusals():
    from qqq_amd.quant import gptq_quantize_ordered, ops

    W, H = torch.zeros((64, 128)), torch.zeros((128, 128))
    with pytest.raises(NotImplementedError, match="gptq_quantize_ordered.*static_groups"):
        gptq_quantize_ordered(W, H, group_size=128, act_order=True, static_groups=False)
    with pytest.raises(NotImplementedError, match="gptq_quantize_ordered"):
        gptq_quantize_ordered(W, H, group_size=64)
    for kw in (dict(), dict(group_size=128), dict(group_size=128, act_order=False), dict(static_groups=False),
               dict(act_order=False, static_groups=False), dict(group_size=128, act_order=False, static_groups=False)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            gptq_quantize_ordered(W, H, **kw)
    with pytest.raises(RuntimeError, match="group_scales: W must be a float32 matrix"):
        ops.group_scales(W.half())
    with pytest.raises(RuntimeError, match="group_scales: every tensor must be on the GPU"):
        ops.group_scales(W)
    with pytest.raises(RuntimeError, match="group_scales: W has 192 columns"):
        ops.group_scales(torch.zeros((4, 192)))
    S, gidx = torch.ones((64, 3)), torch.zeros(128, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="gptq_block_cols: W1 must have 64 or 128 columns"):
        ops.gptq_block_cols(torch.zeros((4, 96)), H, S, gidx)
    with pytest.raises(RuntimeError, match="gptq_block_cols: Hinv1"):
        ops.gptq_block_cols(W, torch.zeros((64, 64)), S, gidx)
    with pytest.raises(RuntimeError, match="gptq_block_cols: scales must have one row per row"):
        ops.gptq_block_cols(W, H, S[:63], gidx)
    with pytest.raises(RuntimeError, match="gptq_block_cols: scales must have unit column stride"):
        ops.gptq_block_cols(W, H, torch.ones((3, 64)).t(), gidx)
    for bad in (gidx.long(), gidx[:64], torch.zeros(256, dtype=torch.int32)[::2], gidx.tolist()):
        with pytest.raises(RuntimeError, match="gptq_block_cols: gidx must be contiguous int32"):
            ops.gptq_block_cols(W, H, S, bad)
    with pytest.raises(RuntimeError, match="gptq_block_cols: every tensor must be on the GPU"):
        ops.gptq_block_cols(W, H, S, gidx)
