"""Rotation at hidden sizes K * 2^p without a GPU: the CPU restatement (tests/rotate_k_ref.py) against the fixture recorded from the
reference's own rotation (tests/golden/rotate_k_small.npz, gen_rotate_k_golden.py) -- its Q and its Q-stage weights, with the reference's
table recovered from the recorded Q --, the tables built here, the factorisation rule, the dense matrix, and every refusal of the new
wrappers, of the new mode and of the entry point, by message."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rotate_k_ref as RK
import rotate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIDDEN, HEAD_DIM, K = 96, 16, 12
CONFIG = dict(model_type="qwen2", vocab_size=48, hidden_size=96, num_attention_heads=6, num_key_value_heads=2, intermediate_size=64,
              num_hidden_layers=2, rms_norm_eps=1e-6, rope_theta=10000.0)
CASES = ((112, 28), (160, 40), (24, 12), (12, 12), (20, 20))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _distance(mine, theirs):
    """(elements whose bits differ, the largest difference among them in fp16 ulps)"""
    diff = _bits(mine) != _bits(theirs)
    if not diff.any():
        return 0, 0.0
    ulp = np.spacing(np.maximum(np.abs(mine), np.abs(theirs)).astype(np.float16)).astype(np.float64)
    return int(diff.sum()), float((np.abs(mine.astype(np.float64) - theirs.astype(np.float64)) / ulp)[diff].max())


@pytest.fixture(scope="module")
def fx():
    g = np.load(os.path.join(ROOT, "tests", "golden", "rotate_k_small.npz"))
    stage = lambda tag: {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "/")}
    orig = stage("orig")
    fused = dict(orig, **stage("fused"))
    rotq = dict(fused, **stage("rotq"))
    return SimpleNamespace(g=g, orig=orig, fused=fused, rotq=rotq, signs=g["signs"], table=RK.recover_table(g["Q"], g["signs"], K))


def test_fixture_is_the_model_the_issue_describes(fx):
    assert fx.orig["model.embed_tokens.weight"].shape == (48, 96) and fx.orig["lm_head.weight"].shape == (48, 96)
    assert fx.orig["model.layers.1.self_attn.q_proj.weight"].shape == (96, 96) and fx.orig["model.layers.1.self_attn.v_proj.weight"].shape == (32, 96)
    assert fx.orig["model.layers.0.mlp.down_proj.weight"].shape == (96, 64) and "model.layers.2.mlp.down_proj.weight" not in fx.orig
    assert all(v.dtype == np.float16 for v in fx.orig.values())
    assert fx.signs.dtype == np.int8 and fx.signs.shape == (96,) and set(fx.signs.tolist()) == {-1, 1}
    assert fx.g["Q"].dtype == np.float64 and fx.g["Q"].shape == (96, 96)
    assert sum(k.startswith("fused/") for k in fx.g.files) == 2 * 5 + 1 + 2 * 2 + 1
    assert sum(k.startswith("rotq/") for k in fx.g.files) == 2 * 7 + 2
    for n, _ in CASES:
        assert fx.g[f"had{n}/W"].shape == (32, n) and fx.g[f"had{n}/W"].dtype == np.float16 and fx.g[f"had{n}/Q"].shape == (n, n)
    # the signs are NOT the sign of Q's first column here: row 0 of the reference's tables is not all ones
    assert not np.array_equal(np.sign(fx.g["Q"][:, 0]).astype(np.int8), fx.signs)


def test_recovered_tables_are_hadamard_and_give_the_reference_q_back(fx):
    cases = [(fx.g["Q"], fx.signs, K)] + [(fx.g[f"had{n}/Q"], fx.g[f"had{n}/signs"], k) for n, k in CASES]
    for Q, signs, k in cases:
        n = Q.shape[0]
        table = RK.recover_table(Q, signs, k)
        t = table.astype(np.int64)
        assert table.dtype == np.int8 and np.array_equal(t @ t.T, k * np.eye(k, dtype=np.int64)), n
        assert not (table[0] == 1).all(), n  # the index order matters: no normalised first row
        assert _same(RK.hadamard_matrix_k(signs, table, n // k), Q), n
    # one table per order, whatever m it was recorded at
    assert np.array_equal(fx.table, RK.recover_table(fx.g["had24/Q"], fx.g["had24/signs"], 12))
    assert np.array_equal(fx.table, RK.recover_table(fx.g["had12/Q"], fx.g["had12/signs"], 12))


def test_restatement_reproduces_the_q_stage(fx):
    """The reference rounds every product of its f64 matmul, the op divides the exact sum once: the generator counted the fp16 elements
    where the two differ (0 in every case on this fixture); no more may differ here, and none by more than one ulp."""
    mine = RK.rotate_q(fx.fused, HIDDEN, fx.signs, fx.table)
    bad, worst = 0, 0.0
    for k in mine:
        b, w = _distance(mine[k], fx.rotq[k])
        bad, worst = bad + b, max(worst, w)
    print(f"model: {bad} elements differ (recorded {int(fx.g['mismatches/model'])}), worst {worst} ulp")
    assert bad == int(fx.g["mismatches/model"]) and worst <= 1 and int(fx.g["max_ulp/model"]) <= 1
    for n, k in CASES:
        tag = f"had{n}"
        table = RK.recover_table(fx.g[tag + "/Q"], fx.g[tag + "/signs"], k)
        b, w = _distance(RK.hadamard_rows_k(fx.g[tag + "/W"], n // k, table, fx.g[tag + "/signs"]), fx.g[tag + "/out"])
        print(f"{tag}: {b} elements differ (recorded {int(fx.g['mismatches/' + tag])}), worst {w} ulp")
        assert b == int(fx.g["mismatches/" + tag]) and w <= 1 and int(fx.g["max_ulp/" + tag]) <= 1


def test_restatement_is_the_power_of_two_op_where_the_table_is_sylvester():
    """K = 4 with the Sylvester table of order 4 and m = 16 is H_64 with the index bits in the same order: the same adds"""
    rng = np.random.Generator(np.random.PCG64(4))
    x = rng.standard_normal((5, 128)).astype(np.float32)
    s = (rng.integers(0, 2, size=64) * 2 - 1).astype(np.int8)
    h4 = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], np.int8)
    # the last two stages of H_64 are ((a + b) + (c + d)); the mix adds ((a + b) + c) + d: the same for fp16 (exact), not for f32
    x16 = x.astype(np.float16)
    assert _same(RK.hadamard_rows_k(x16, 16, h4, s), R.hadamard_rows(x16, 64, s))
    assert np.allclose(RK.hadamard_rows_k(x, 16, h4, s), R.hadamard_rows(x, 64, s), rtol=1e-6, atol=1e-6)


def test_tables_built_here_are_hadamard():
    from qqq_amd.quant import hadamard_table

    for k in (12, 20, 28, 40):
        t = hadamard_table(k)
        assert t.dtype == torch.int8 and tuple(t.shape) == (k, k) and t.is_contiguous() and bool((t.abs() == 1).all())
        t64 = t.to(torch.int64)
        assert torch.equal(t64 @ t64.t(), k * torch.eye(k, dtype=torch.int64)), k
        assert torch.equal(t, hadamard_table(k))  # by construction: the same every time
    for k in (4, 16, 24, 36, 44, 0):
        with pytest.raises(RuntimeError, match=f"hadamard_table: no table of order K = {k} "):
            hadamard_table(k)


def test_tables_built_here_are_not_the_references(fx):
    from qqq_amd.quant import hadamard_table

    for tag, k in (("had12", 12), ("had20", 20), ("had112", 28), ("had160", 40)):
        theirs = RK.recover_table(fx.g[tag + "/Q"], fx.g[tag + "/signs"], k)
        ours = hadamard_table(k).numpy()
        assert not any(np.array_equal(ours, m) for m in (theirs, theirs.T, -theirs, -theirs.T)), k


def test_hadamard_factor_follows_the_references_precedence():
    from qqq_amd.quant import hadamard_factor

    want = {896: (28, 32), 1536: (12, 128), 3072: (12, 256), 3584: (28, 128), 5120: (40, 128), 4096: (1, 4096), 96: (12, 8), 20: (20, 1),
            40: (40, 1), 64: (1, 64), 12: (12, 1), 28: (28, 1), 80: (40, 2), 160: (40, 4)}
    for n, km in want.items():
        assert hadamard_factor(n) == km, n
    with pytest.raises(RuntimeError, match="hadamard_factor: n = 4608 is a multiple of 36.*table="):
        hadamard_factor(4608)
    with pytest.raises(RuntimeError, match="hadamard_factor: n = 100 = 20 \\* 5, and 5 is not a power of two.*table="):
        hadamard_factor(100)
    for n, k in ((36, 36), (52, 52), (60, 60), (108, 108), (140, 140), (156, 156), (172, 172), (13824, 108), (11008, 172)):
        with pytest.raises(RuntimeError, match=f"hadamard_factor: n = {n} is a multiple of {k}.*table="):
            hadamard_factor(n)
    with pytest.raises(RuntimeError, match="hadamard_factor: n = 84 = 28 \\* 3, and 3 is not a power of two"):
        hadamard_factor(84)  # 28 before 12 (84 = 12 * 7 as well), as the reference, which then asserts
    with pytest.raises(RuntimeError, match="hadamard_factor: n = 280 is a multiple of 140"):
        hadamard_factor(280)  # every common multiple of 28 and 40 is one of 140
    with pytest.raises(RuntimeError, match="hadamard_factor: n = 7 is neither"):
        hadamard_factor(7)
    with pytest.raises(RuntimeError, match="hadamard_factor: n must be a positive integer"):
        hadamard_factor(0)


def test_hadamard_matrix_k(fx):
    """The matrix is diag(s) (table^T (x) H_m) / d with d = sqrt(n) in f32, as the op and the reference: Q Q^T = (n / d^2) I.  Its rows
    are orthogonal to 1e-12 at every size; its diagonal is 1 to 1e-12 where d is exact (n a power of four: caller's tables of order 4
    and 16), and n / d^2 = 1 +- 6e-8 at the shipped orders, where n is no square -- the reference's own Q has the same diagonal."""
    from qqq_amd.quant import hadamard_matrix_k, hadamard_signs, hadamard_table

    h4 = torch.tensor([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], dtype=torch.int8)
    h16 = torch.kron(h4.long(), h4.long()).to(torch.int8)
    for table, m in ((h4, 4), (h4, 16), (h16, 4), (h16, 1)):
        n = table.shape[0] * m
        Q = hadamard_matrix_k(hadamard_signs(n, torch.Generator().manual_seed(n)), table, m)
        assert Q.dtype == torch.float64 and float((Q @ Q.T - torch.eye(n, dtype=torch.float64)).abs().max()) <= 1e-12, n
    for k, m in ((12, 8), (20, 1), (28, 4), (40, 4), (12, 1), (28, 32)):
        n = k * m
        s = hadamard_signs(n, torch.Generator().manual_seed(n))
        Q = hadamard_matrix_k(s, hadamard_table(k), m)
        d = float(R.divisor(n))
        G = Q @ Q.T
        off = G - torch.diag(torch.diag(G))
        print(f"n = {n}: off-diagonal {float(off.abs().max()):.2e}, diagonal - 1 = {float((torch.diag(G) - 1).abs().max()):.2e}")
        assert float(off.abs().max()) <= 1e-12 and float((torch.diag(G) - n / d ** 2).abs().max()) <= 1e-12, n
        assert abs(n / d ** 2 - 1) < 2.0 ** -23
        assert _same(Q.numpy(), RK.hadamard_matrix_k(s.numpy(), hadamard_table(k).numpy(), m)), n
    # the fixture's Q, bit for bit, from the recovered table
    assert _same(hadamard_matrix_k(torch.from_numpy(fx.signs), torch.from_numpy(fx.table), 8).numpy(), fx.g["Q"])
    for n, k in CASES:
        table = RK.recover_table(fx.g[f"had{n}/Q"], fx.g[f"had{n}/signs"], k)
        assert _same(hadamard_matrix_k(torch.from_numpy(fx.g[f"had{n}/signs"]), torch.from_numpy(table), n // k).numpy(), fx.g[f"had{n}/Q"]), n
    Qf = fx.g["Q"]
    assert abs(float((Qf @ Qf.T)[0, 0]) - 96 / float(R.divisor(96)) ** 2) <= 1e-12
    with pytest.raises(RuntimeError, match="hadamard_matrix_k: 64 signs for n = 12 \\* 8 = 96"):
        hadamard_matrix_k(torch.ones(64, dtype=torch.int8), hadamard_table(12), 8)


def test_the_dense_matrix_is_what_the_restatement_multiplies_by(fx):
    """x . Q in exact arithmetic against the restatement: fp16 inputs, every sum exact, so only the divide's rounding is between them"""
    from qqq_amd.quant import hadamard_matrix_k, hadamard_table

    rng = np.random.Generator(np.random.PCG64(11))
    for k, m in ((12, 8), (28, 4), (40, 2), (20, 1)):
        n = k * m
        x = rng.standard_normal((7, n)).astype(np.float16)
        s = (rng.integers(0, 2, size=n) * 2 - 1).astype(np.int8)
        table = hadamard_table(k)
        Q = hadamard_matrix_k(torch.from_numpy(s), table, m).numpy()
        want = x.astype(np.float64) @ Q
        got = RK.mix_f64(x, table.numpy(), m, s)
        assert np.allclose(got, want, rtol=1e-13, atol=1e-13), n


def test_wrappers_refuse_before_anything_reaches_the_library(fx):
    from qqq_amd.quant import check_table, hadamard_rows_k, hadamard_table, ops

    t12 = hadamard_table(12)
    assert check_table(t12) is t12 and ops.check_table is check_table
    bad = t12.clone()
    bad[3, 4] = 0
    flipped = t12.clone()
    flipped[3, 4] = -flipped[3, 4]
    for table, msg in ((t12.float(), "check_table: table must be contiguous int8 \\[K, K\\], got float32 \\(12, 12\\)"),
                       (t12[:, :8], "check_table: table must be contiguous int8 \\[K, K\\]"),
                       (t12.t(), "check_table: table must be contiguous int8 \\[K, K\\]"),
                       (t12[0], "check_table: table must be contiguous int8 \\[K, K\\]"),
                       ([[1]], "check_table: table must be contiguous int8 \\[K, K\\], got list"),
                       (torch.ones((6, 6), dtype=torch.int8), "check_table: table has K = 6, no multiple of 4 in 4 ... 64"),
                       (torch.ones((68, 68), dtype=torch.int8), "check_table: table has K = 68, no multiple of 4 in 4 ... 64"),
                       (torch.ones((0, 0), dtype=torch.int8), "check_table: table has K = 0"),
                       (bad, "check_table: every entry of table must be \\+1 or -1"),
                       (flipped, "check_table: table is no Hadamard matrix \\(table . table\\^T != 12 I\\)"),
                       (torch.ones((8, 8), dtype=torch.int8), "check_table: table is no Hadamard matrix")):
        with pytest.raises(RuntimeError, match=msg):
            check_table(table)
    with pytest.raises(RuntimeError, match="mine: every entry of table"):
        check_table(bad, "mine")
    x = torch.zeros((4, 96), dtype=torch.float16)
    for kw, msg in ((dict(x=x.double(), m=8, table=t12), "hadamard_rows_k: x must be a float16 or float32 matrix"),
                    (dict(x=x[0], m=8, table=t12), "hadamard_rows_k: x must be a float16 or float32 matrix"),
                    (dict(x=x.t(), m=1, table=t12), "unit column stride"),
                    (dict(x=x, m=8, table=t12.long()), "hadamard_rows_k: table must be contiguous int8 \\[K, K\\], got int64"),
                    (dict(x=x, m=8, table=torch.ones((6, 6), dtype=torch.int8)), "hadamard_rows_k: table has K = 6"),
                    (dict(x=x, m=3, table=t12), "hadamard_rows_k: m must be a power of two with K \\* m = 12 \\* m <= 8192, got 3"),
                    (dict(x=x, m=0, table=t12), "hadamard_rows_k: m must be a power of two"),
                    (dict(x=x, m=8.0, table=t12), "hadamard_rows_k: m must be a power of two"),
                    (dict(x=x, m=1024, table=t12), "hadamard_rows_k: m must be a power of two with K \\* m = 12 \\* m <= 8192, got 1024"),
                    (dict(x=x, m=16, table=t12), "hadamard_rows_k: x has 96 columns, no multiple of n = 192"),
                    (dict(x=x, m=8, table=t12, out=torch.zeros((4, 96))), "hadamard_rows_k: out must be a float16 matrix"),
                    (dict(x=x, m=8, table=t12, out=torch.zeros((4, 48), dtype=torch.float16)), "hadamard_rows_k: out has the shape"),
                    (dict(x=x, m=8, table=t12, sign=torch.ones(96)), "hadamard_rows_k: sign must be contiguous int8 \\[96\\]"),
                    (dict(x=x, m=8, table=t12, sign=torch.ones(64, dtype=torch.int8)), "hadamard_rows_k: sign must be contiguous int8 \\[96\\]"),
                    (dict(x=x, m=8, table=t12), "hadamard_rows_k: every tensor must be on the GPU")):
        with pytest.raises(RuntimeError, match=msg):
            hadamard_rows_k(**kw)


def test_the_new_mode_refuses_what_it_cannot_do(fx):
    from qqq_amd.quant import hadamard_table, quantize_model, rotate_model, rotate_state_dict

    sd = {k: torch.from_numpy(v.copy()) for k, v in fx.fused.items()}
    cfg = SimpleNamespace(**CONFIG)
    t12, t20 = hadamard_table(12), hadamard_table(20)
    # mode="hadamard" keeps its refusal of hidden 96, and now says where to go
    with pytest.raises(RuntimeError, match="rotate_state_dict: hidden_size = 96 is not a power of two.*Paley.*mode='hadamard_k'.*mode='random'"):
        rotate_state_dict(sd, cfg)
    with pytest.raises(RuntimeError, match="rotate_state_dict: mode must be 'hadamard', 'hadamard_k' or 'random', got 'paley'"):
        rotate_state_dict(sd, cfg, mode="paley")
    for kw in (dict(mode="hadamard"), dict(mode="random"), dict(mode="hadamard_k", Q=torch.eye(96, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="rotate_state_dict: table belongs to mode='hadamard_k' without an explicit Q"):
            rotate_state_dict(sd, cfg, table=t12, **kw)
    with pytest.raises(RuntimeError, match="rotate_state_dict: hidden_size = 96 is not the table's order 20 times a power of two"):
        rotate_state_dict(sd, cfg, mode="hadamard_k", table=t20)
    with pytest.raises(RuntimeError, match="rotate_state_dict: every entry of table must be"):
        rotate_state_dict(sd, cfg, mode="hadamard_k", table=torch.zeros((12, 12), dtype=torch.int8))
    with pytest.raises(RuntimeError, match="rotate_state_dict: table is no Hadamard matrix"):
        rotate_state_dict(sd, cfg, mode="hadamard_k", table=torch.ones((12, 12), dtype=torch.int8))
    with pytest.raises(RuntimeError, match="rotate_state_dict: table must be contiguous int8"):
        rotate_state_dict(sd, cfg, mode="hadamard_k", table=t12.float())
    with pytest.raises(RuntimeError, match="rotate_state_dict: sign must be contiguous int8 \\[96\\]"):
        rotate_state_dict(sd, cfg, mode="hadamard_k", signs=torch.ones(64, dtype=torch.int8))
    zero = torch.ones(96, dtype=torch.int8)
    zero[5] = 0
    with pytest.raises(RuntimeError, match="rotate_state_dict: every entry of sign must be"):
        rotate_state_dict(sd, cfg, mode="hadamard_k", signs=zero)
    # sizes: the reference's other tables by name, no power of two, too large; the per-head step still needs a power of two
    for hidden, heads, msg in ((576, 36, "rotate_state_dict: hidden_size: hadamard_factor: n = 576 is a multiple of 36.*table="),
                               (1600, 100, "rotate_state_dict: hidden_size: hadamard_factor: n = 1600 = 40 \\* 40, and 40 is not a power"),
                               (176, 11, "rotate_state_dict: hidden_size: hadamard_factor: n = 176 is neither"),
                               (10240, 640, "rotate_state_dict: hidden_size = 10240 is not in 1 ... 8192"),
                               (96, 4, "rotate_state_dict: head_dim = 24 is not a power of two")):
        with pytest.raises(RuntimeError, match=msg):
            rotate_state_dict(sd, SimpleNamespace(**dict(CONFIG, hidden_size=hidden, num_attention_heads=heads)), mode="hadamard_k")
    with pytest.raises(RuntimeError, match="rotate_state_dict: the state dict has no lm_head.weight"):
        rotate_state_dict({k: v for k, v in sd.items() if k != "lm_head.weight"}, cfg, mode="hadamard_k")
    with pytest.raises(RuntimeError, match="is bfloat16"):
        rotate_model({k: torch.from_numpy(v.copy()).bfloat16() for k, v in fx.orig.items()}, cfg, mode="hadamard_k")
    for rotation in (3, ("hadamard_k",), ("hadamard", torch.ones(96, dtype=torch.int8)), ("hadamard_k", [1] * 96)):
        with pytest.raises(RuntimeError, match="quantize_model: rotation must be None, 'hadamard', 'hadamard_k', 'random', a tensor"):
            quantize_model(sd, cfg, torch.zeros((1, 8), dtype=torch.int64), -1, rotation=rotation)


def test_rotate_k_header_binds_beside_the_others():
    from qqq_amd import _abi, build
    from qqq_amd.quant import _lib as qlib

    L = qlib.lib()
    header = os.path.join(build.QUANT_EXT_INCLUDE, "qqq_amd_rotate_k.h")
    protos = _abi.prototypes(header)
    assert set(protos) == {"qqq_hadamard_rows_k"}
    ret, params = protos["qqq_hadamard_rows_k"]
    assert ret == "int" and len(params) == 13 and len(L.qqq_hadamard_rows_k.argtypes) == 13
    assert all(_abi.ctype_of(p) in (ctypes.c_void_p, ctypes.c_int) for p in params)
    # quant/include/ is pinned to its three headers: this one is in the quantiser's second flat directory, listed, watched and bound
    assert build.QUANT_EXT_INCLUDE == os.path.join(ROOT, "qqq_amd", "quant", "include_ext")
    assert build.quant_ext_headers() == [header] and header not in build.quant_headers()
    assert [d for d in os.listdir(build.QUANT_EXT_INCLUDE) if os.path.isdir(os.path.join(build.QUANT_EXT_INCLUDE, d))] == []
    seen = {}
    for h in build.quant_headers() + build.quant_ext_headers():  # bound onto one handle: no name twice
        for name in _abi.prototypes(h):
            assert name not in seen, (name, seen[name], h)
            seen[name] = h
    # the headers of quant/include/ keep what they had, and the pinned ABI version stays
    assert set(_abi.prototypes(os.path.join(build.QUANT_INCLUDE, "qqq_amd_rotate.h"))) == {"qqq_hadamard_rows"}
    assert "qqq_hadamard_rows_k" not in _abi.prototypes(build.QUANT_HEADER) and L.qqq_quant_abi_version() == 1


def test_a_newer_rotate_k_header_rebuilds_the_quantiser_library(monkeypatch):
    """build_quant returns early when the library is the newest file and compiles when this header is newer (nothing is compiled here)"""
    from qqq_amd import build

    build.build_quant()  # the library exists
    newer = os.path.join(build.QUANT_EXT_INCLUDE, "qqq_amd_rotate_k.h")
    compiled = []
    monkeypatch.setattr(build, "_compile", lambda src, out, verbose, flags=(): compiled.append((src, out, tuple(flags))) or out)
    monkeypatch.setattr(os.path, "getmtime", lambda p: 2.0 if p == build.QUANT_LIB else 1.0)
    assert build.build_quant() == build.QUANT_LIB and not compiled
    monkeypatch.setattr(os.path, "getmtime", lambda p: 2.0 if p == build.QUANT_LIB else 3.0 if p == newer else 1.0)
    assert build.build_quant() == build.QUANT_LIB and compiled == [(build.QUANT_SRC, build.QUANT_LIB, build.QUANT_FLAGS)]


def test_entry_point_refuses_bad_arguments_by_name():
    from qqq_amd.quant import _lib as qlib

    L = qlib.lib()
    buf = (ctypes.c_float * 1024)()
    p = ctypes.addressof(buf)
    q = p + 2048
    table = (ctypes.c_byte * 4096)()
    ok = dict(X=p, ldx=192, Y=q, ldy=192, rows=2, cols=192, K=12, m=8, table=ctypes.addressof(table), sign=None, dtype=0)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.qqq_hadamard_rows_k(a["X"], a["ldx"], a["Y"], a["ldy"], a["rows"], a["cols"], a["K"], a["m"], a["table"], a["sign"], a["dtype"],
                                   0, None)
        return rc, qlib.last_error()

    for kw in (dict(dtype=2), dict(dtype=-1), dict(K=0), dict(K=2), dict(K=6), dict(K=68), dict(K=-12), dict(m=0), dict(m=3), dict(m=-8),
               dict(m=1024), dict(K=64, m=256), dict(m=1 << 30), dict(rows=0), dict(cols=0), dict(cols=100), dict(cols=48), dict(ldx=191),
               dict(ldy=96), dict(X=None), dict(Y=None), dict(table=None), dict(X=p + 1), dict(Y=q + 1), dict(dtype=1, X=p + 2),
               dict(Y=p, ldy=384, ldx=192), dict(Y=p + 64), dict(Y=p + 2 * 200), dict(X=q, Y=p + 2048 - 2 * 100)):
        rc, msg = call(**kw)
        assert rc == qlib.ERR_ARG and msg.startswith("qqq_hadamard_rows_k: "), (kw, rc, msg)
