"""The GPTQ quantiser without a GPU: the CPU restatement (tests/gptq_ref.py) against the fixture recorded from the reference's own
GPTQ.fasterquant (tests/golden/gptq_small.npz, gen_gptq_golden.py), the restatement's shrink search judged in f64, and the quantiser's
library: it loads and binds from its header, leaves the operator library and build.py's listers alone, and refuses bad arguments by name."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gptq_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(-1, False), (-1, True), (128, False), (128, True)]
# the chosen candidate's f64 error may exceed the f64 minimum over the 80 candidates by this relative amount: what an f32 sum of up to
# 28 672 positive terms can move a ranking by (the reference's own choice sits at the f64 optimum on the inputs it was measured on)
MSE_SLACK = 1e-4


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "gptq_small.npz"))
    K = g["W"].shape[1]
    iu = np.triu_indices(K)
    Hinv = np.zeros((K, K), np.float32)
    Hinv[iu] = g["Hinv_triu"]
    H = np.zeros((K, K), np.float32)
    H[iu] = g["H_triu"]
    H = H + np.triu(H, 1).T
    return g, H, Hinv


@pytest.mark.parametrize("gs,mse", SETTINGS)
def test_restatement_reproduces_the_reference_bit_for_bit(fixture, gs, mse):
    g, H, Hinv = fixture
    tag = f"g{gs}_mse{int(mse)}"
    r = R.sweep(g["W"], Hinv, np.diag(H) == 0, gs, mse)
    assert np.array_equal(r["scales"].view(np.int32), g[tag + "/scales"].view(np.int32))
    assert np.array_equal(R.codes(r["weight"], r["scales"], gs != -1), g[tag + "/codes"])
    assert np.array_equal(r["weight"].view(np.int16), g[tag + "/weight"].view(np.int16))
    if gs != -1:
        assert np.array_equal(r["s_extra"].view(np.int32), g[tag + "/s_extra"].view(np.int32))
    lo, hi = (0, 15) if gs != -1 else (-7, 7)
    assert g[tag + "/codes"].min() >= lo and g[tag + "/codes"].max() <= hi


def test_fixture_factor_is_the_cholesky_chain_of_its_hessian(fixture):
    # the factor is stored so that the bit tests do not depend on this machine's LAPACK; it is still the chain's, to rounding
    g, H, Hinv = fixture
    again, dead = R.hinv_of(H)
    assert not dead.any()
    assert np.allclose(np.triu(again), Hinv, rtol=1e-3, atol=1e-6 * np.abs(Hinv).max())


def _mse_inputs(fixture):
    g = fixture[0]
    rng = np.random.Generator(np.random.PCG64(7))
    W = g["W"].astype(np.float32)
    heavy = (rng.standard_t(3, size=(16, 4096)) * 0.01).astype(np.float32)  # outliers: the search shrinks
    return [("golden rows", W, False), ("golden group", W[:, 128:], True), ("16x4096 t3", heavy, False), ("16x4096 t3 g", heavy[:, :128], True)]


def test_restatement_scale_search_is_optimal_in_f64(fixture):
    for name, W, grouped in _mse_inputs(fixture):
        s, idx = R.scales(W, grouped, True, return_index=True)
        err = R.errors_f64(W, grouped)
        chosen, best = err[np.arange(W.shape[0]), idx], err.min(axis=1)
        print(f"{name}: worst chosen / minimum - 1 = {float((chosen / best).max() - 1):.2e}; candidates used {sorted(set(idx.tolist()))[:8]}")
        assert (chosen <= (1 + MSE_SLACK) * best).all(), name
        assert np.array_equal(s.view(np.int32), R.candidates(W, grouped)[np.arange(W.shape[0]), idx].view(np.int32))
    assert len(set(R.scales(_mse_inputs(fixture)[2][1], False, True, return_index=True)[1].tolist())) > 1  # the search does move


def test_restatement_edge_rows():
    W = np.zeros((3, 128), np.float32)
    W[1, 5] = -3.5
    W[2] = np.float32(1e-41)  # subnormal
    for grouped in (False, True):
        s = R.scales(W, grouped)
        assert s[0] == (np.float32(2) / np.float32(15) if grouped else np.float32(1) / np.float32(7))
        assert s[1] == (np.float32(7) / np.float32(15) if grouped else np.float32(0.5))
        assert s[2] > 0 and np.isfinite(R.quantise(W[2], s[2], grouped)).all()
    # ties go to even, the clamp holds on both sides
    assert R.quantise(np.float32([0.5, 1.5, 2.5, -0.5, 100, -100]), np.float32(1), False).tolist() == [0, 2, 2, -0.0, 7, -7]
    assert R.quantise(np.float32([0.5, 1.5, 100, -100]), np.float32(1), True).tolist() == [0, 2, 7, -8]


def test_hessian_counts_samples_as_the_reference():
    from qqq_amd.quant import Hessian

    g = torch.Generator().manual_seed(0)
    x3, x2 = torch.randn((3, 5, 64), generator=g).half(), torch.randn((7, 64), generator=g).half()
    h = Hessian(64, "cpu")
    h.add_batch(x3)  # three samples
    h.add_batch(x2)  # one sample
    assert h.nsamples == 4
    a, b = x3.reshape(-1, 64).double(), x2.double()
    want = (2 / 3 * a.t() @ a) * (3 / 4) + 2 / 4 * b.t() @ b
    assert torch.allclose(h.H.double(), want, rtol=1e-5, atol=1e-5)
    with pytest.raises(RuntimeError, match="add_batch"):
        h.add_batch(torch.zeros(2, 32))


def test_library_loads_and_binds_from_its_header_beside_the_operator():
    from qqq_amd import _abi, _lib, build
    from qqq_amd.quant import _lib as qlib

    L = qlib.lib()
    protos = _abi.prototypes(build.QUANT_HEADER)
    assert set(protos) == {"qqq_quant_abi_version", "qqq_quant_last_error", "qqq_gptq_scales", "qqq_gptq_block"}
    for name, (_, params) in protos.items():
        assert len(getattr(L, name).argtypes or []) == len(params), name
        for p in params:  # only the parameter types the operator's headers already use
            assert _abi.ctype_of(p) in (ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t), p
    assert L.qqq_quant_abi_version() == qlib.ABI_VERSION == 1
    # the operator library and its lister do not know the quantiser
    assert _lib.lib().qqq_amd_abi_version() == _lib.ABI_VERSION == 4
    assert not hasattr(_lib.lib(), "qqq_gptq_block")
    inc = os.path.join(ROOT, "include") + os.sep
    every = build.headers()
    assert every and all(h.startswith(inc) for h in every)
    assert build.QUANT_HEADER in build.quant_headers() and not any(h.startswith(inc) for h in build.quant_headers())
    found = sorted(os.path.join(top, f) for top, _, fs in os.walk(inc) for f in fs if f.endswith(".h"))
    assert every == found
    assert os.path.basename(build.QUANT_LIB) == "libqqq_amd_quant.so" and build.LIB != build.QUANT_LIB


def _quant_headers():
    inc = os.path.join(ROOT, "qqq_amd", "quant", "include")
    return sorted(f for f in os.listdir(inc) if f.endswith(".h"))


def test_quant_headers_are_found_by_listing_the_quant_include_directory():
    from qqq_amd import build

    assert _quant_headers() == ["qqq_amd_gptq_order.h", "qqq_amd_quant.h", "qqq_amd_rotate.h"]
    assert build.quant_headers() == [os.path.join(ROOT, "qqq_amd", "quant", "include", h) for h in _quant_headers()]


@pytest.mark.parametrize("header", _quant_headers())
def test_a_newer_header_rebuilds_the_quantiser_library(monkeypatch, header):
    """build_quant returns early when the library is the newest file and compiles when this one header is newer (nothing is compiled here)"""
    from qqq_amd import build

    build.build_quant()  # the library exists
    newer = os.path.join(ROOT, "qqq_amd", "quant", "include", header)
    compiled = []
    monkeypatch.setattr(build, "_compile", lambda src, out, verbose, flags=(): compiled.append((src, out, tuple(flags))) or out)
    monkeypatch.setattr(os.path, "getmtime", lambda p: 2.0 if p == build.QUANT_LIB else 1.0)
    assert build.build_quant() == build.QUANT_LIB and not compiled
    monkeypatch.setattr(os.path, "getmtime", lambda p: 2.0 if p == build.QUANT_LIB else 3.0 if p == newer else 1.0)
    assert build.build_quant() == build.QUANT_LIB and compiled == [(build.QUANT_SRC, build.QUANT_LIB, build.QUANT_FLAGS)]


def _refused(fn, *args):
    from qqq_amd.quant import _lib as qlib

    rc = fn(*args)
    return rc, qlib.last_error()


def test_entry_points_refuse_bad_arguments_by_name():
    from qqq_amd.quant import _lib as qlib

    L = qlib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok_block = dict(W1=p, ldw=128, Hinv1=p, ldh=128, scale=p, rows=4, count=128, grouped=0, Q1=p, ldq=128, Err1=p, lde=128)

    def block(**kw):
        a = dict(ok_block, **kw)
        return _refused(L.qqq_gptq_block, a["W1"], a["ldw"], a["Hinv1"], a["ldh"], a["scale"], a["rows"], a["count"], a["grouped"], a["Q1"],
                        a["ldq"], a["Err1"], a["lde"], 0, None)

    for kw in (dict(count=96), dict(count=0), dict(rows=0), dict(ldw=127), dict(ldh=64), dict(ldq=100), dict(lde=1), dict(grouped=2),
               dict(W1=None), dict(Hinv1=None), dict(scale=None), dict(Q1=None), dict(Err1=None), dict(W1=p + 2), dict(Err1=p + 1)):
        rc, msg = block(**kw)
        assert rc == qlib.ERR_ARG and msg.startswith("qqq_gptq_block: "), (kw, rc, msg)

    ok_scales = dict(W=p, ldw=128, rows=4, cols=128, grouped=0, mse=0, out=p)

    def scales(**kw):
        a = dict(ok_scales, **kw)
        return _refused(L.qqq_gptq_scales, a["W"], a["ldw"], a["rows"], a["cols"], a["grouped"], a["mse"], a["out"], 0, None)

    for kw in (dict(rows=0), dict(cols=0), dict(cols=1 << 21, ldw=1 << 21), dict(ldw=64), dict(grouped=-1), dict(mse=3), dict(W=None),
               dict(out=None), dict(W=p + 1), dict(out=p + 2)):
        rc, msg = scales(**kw)
        assert rc == qlib.ERR_ARG and msg.startswith("qqq_gptq_scales: "), (kw, rc, msg)


def test_python_layer_refuses_what_pack_cannot_hold():
    from qqq_amd.quant import gptq_quantize, ops

    W, H = torch.zeros((64, 128)), torch.zeros((128, 128))
    for kw in (dict(act_order=True), dict(static_groups=True), dict(sym=False), dict(bits=3), dict(bits=8), dict(group_size=64), dict(group_size=32)):
        with pytest.raises(NotImplementedError, match="gptq_quantize"):
            gptq_quantize(W, H, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gptq_quantize(W, H)
    with pytest.raises(RuntimeError, match="weight_scales: W must be a float32 matrix"):
        ops.weight_scales(W.half(), False)
    with pytest.raises(RuntimeError, match="weight_scales: every tensor must be on the GPU"):
        ops.weight_scales(W, False)
    with pytest.raises(RuntimeError, match="gptq_block: W1 must have 64 or 128 columns"):
        ops.gptq_block(torch.zeros((4, 96)), H, torch.ones(4), False)
    with pytest.raises(RuntimeError, match="gptq_block: Hinv1"):
        ops.gptq_block(W, torch.zeros((64, 64)), torch.ones(64), False)
    with pytest.raises(RuntimeError, match="gptq_block: scale"):
        ops.gptq_block(W, H, torch.ones(63), False)
    with pytest.raises(RuntimeError, match="unit column stride"):
        ops.gptq_block(torch.zeros((128, 64)).t(), H, torch.ones(64), False)
