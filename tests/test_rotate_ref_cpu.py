"""Rotation without a GPU: the CPU restatement (tests/rotate_ref.py) against the fixture recorded from the reference's own rotation
(tests/golden/rotate_small.npz, gen_rotate_golden.py) -- its Q, its fused weights and its Q-stage weights bit for bit, its per-head stage
(a stand-in there: the CUDA package is missing) within the recorded count -- the invariance of the model's function under an f64
forward, the torch fuse step against the restatement, and the library: the new header binds and the entry point refuses bad arguments
by name."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rotate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIDDEN, HEAD_DIM = 64, 16
CONFIG = dict(model_type="qwen2", vocab_size=96, hidden_size=64, num_attention_heads=4, num_key_value_heads=2, intermediate_size=128,
              num_hidden_layers=2, rms_norm_eps=1e-6, rope_theta=10000.0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def fx():
    """the fixture as four whole state dicts (every stage stores only what it changed) and the rest"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "rotate_small.npz"))
    stage = lambda tag: {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "/")}
    orig = stage("orig")
    fused = dict(orig, **stage("fused"))
    rotq = dict(fused, **stage("rotq"))
    full = dict(rotq, **stage("full_standin"))
    return SimpleNamespace(g=g, orig=orig, fused=fused, rotq=rotq, full=full, signs=g["signs"])


def test_fixture_is_the_model_the_issue_describes(fx):
    assert fx.orig["model.embed_tokens.weight"].shape == (96, 64) and fx.orig["lm_head.weight"].shape == (96, 64)
    assert fx.orig["model.layers.1.self_attn.v_proj.weight"].shape == (32, 64) and "model.layers.1.self_attn.v_proj.bias" in fx.orig
    assert fx.orig["model.layers.0.mlp.down_proj.weight"].shape == (64, 128) and "model.layers.2.mlp.down_proj.weight" not in fx.orig
    assert all(v.dtype == np.float16 for v in fx.orig.values())
    assert fx.signs.dtype == np.int8 and set(fx.signs.tolist()) == {-1, 1} and fx.g["Q"].dtype == np.float64
    # every stage changed what it should and nothing else
    assert sum(k.startswith("fused/") for k in fx.g.files) == 2 * 5 + 1 + 2 * 2 + 1  # q k v gate up, lm_head; the norms
    assert sum(k.startswith("rotq/") for k in fx.g.files) == 2 * 7 + 2
    assert sorted(k.split(".", 3)[3] for k in fx.g.files if k.startswith("full_standin/model.layers.0.")) == [
        "self_attn.o_proj.weight", "self_attn.v_proj.bias", "self_attn.v_proj.weight"]


def test_restatement_reproduces_the_reference_q(fx):
    assert _same(R.hadamard_matrix(fx.signs), fx.g["Q"])
    assert _same(R.hadamard_matrix(fx.g["had128/signs"]), fx.g["had128/Q"])
    Q = fx.g["Q"]
    assert np.allclose(Q @ Q.T, np.eye(HIDDEN), atol=1e-12)


def test_restatement_reproduces_the_fused_weights(fx):
    mine = R.fuse_layer_norms(fx.orig)
    assert sorted(mine) == sorted(fx.fused)
    for k in mine:
        assert _same(mine[k], fx.fused[k]), k
    assert all((mine[k] == 1).all() for k in mine if k.endswith("norm.weight"))


def test_restatement_reproduces_the_q_stage_bit_for_bit(fx):
    mine = R.rotate_q(fx.fused, HIDDEN, fx.signs)
    for k in mine:
        assert _same(mine[k], fx.rotq[k]), k
    # n = 128: the divisor is no power of two, the reference's matmul rounds per product and we divide the exact sum once
    assert _same(R.hadamard_rows(fx.g["had128/W"], 128, fx.g["had128/signs"]), fx.g["had128/out"])


def test_full_stage_is_within_the_recorded_distance_of_the_stand_in(fx):
    """full_standin/ is an f32 product with the Sylvester matrix in place of the reference's CUDA package; the generator counted how many
    elements differ from the exact sum rounded once (0 on this fixture) and by how many fp16 ulps at most"""
    mine = R.rotate_ov(fx.rotq, HEAD_DIM)
    bad, worst = 0, 0.0
    for k in mine:
        diff = _bits(mine[k]) != _bits(fx.full[k])
        bad += int(diff.sum())
        if diff.any():
            ulp = np.spacing(np.maximum(np.abs(mine[k]), np.abs(fx.full[k])).astype(np.float16)).astype(np.float64)
            worst = max(worst, float((np.abs(mine[k].astype(np.float64) - fx.full[k].astype(np.float64)) / ulp)[diff].max()))
    print(f"elements that differ from the stand-in: {bad} (recorded {int(fx.g['standin_mismatches'])}), worst {worst} ulp")
    assert bad <= int(fx.g["standin_mismatches"]) and worst <= 1
    assert int(fx.g["standin_max_ulp"]) <= 1


def test_the_double_rounding_is_part_of_the_restatement():
    # (2 + 2^-10 + 2^-24) / 2 = 1 + 2^-11 + 2^-25: f32 drops the last term, the tie then goes to even; one rounding would go up
    x = np.zeros((1, 4), np.float16)
    x[0, :3] = [2.0, 2.0 ** -10, 2.0 ** -24]
    assert x[0, 2] > 0
    y = R.hadamard_rows(x, 4)
    assert y[0, 0] == np.float16(1.0)
    assert np.float64(1 + 2.0 ** -11 + 2.0 ** -25).astype(np.float16) == np.float16(1 + 2.0 ** -10)
    assert torch.tensor([1 + 2.0 ** -11 + 2.0 ** -25], dtype=torch.float64).half().item() == 1.0  # torch rounds twice as well


def _logits(sd, ids):
    """f64 forward of the float model on the CPU: FloatDecoderLayer per layer, the final norm, the head"""
    from qqq_amd.quant import FloatDecoderLayer
    from qqq_amd.quant.model import _rms_norm

    cfg = SimpleNamespace(**CONFIG)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in sd.items()}
    x = torch.nn.functional.embedding(ids, t["model.embed_tokens.weight"])
    for p in R.layer_prefixes(sd):
        x = FloatDecoderLayer(cfg, {k[len(p):]: v for k, v in t.items() if k.startswith(p)}).forward(x)
    x = _rms_norm(x, t["model.norm.weight"], CONFIG["rms_norm_eps"])
    return x @ t.get("lm_head.weight", t["model.embed_tokens.weight"]).t()


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_rotation_leaves_the_models_function_alone(fx):
    """2 x 16 tokens.  The yardstick is the deviation the REFERENCE's rotated weights (the fixture's) show against the unrotated model
    under the same forward; ours may be twice that: both pipelines round every weight the same number of times."""
    ids = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).integers(0, 96, size=(2, 16)))
    want = _logits(fx.orig, ids)
    ref_dev = _rel(_logits(fx.full, ids), want)
    mine = R.rotate_model(fx.orig, HIDDEN, HEAD_DIM, fx.signs)
    my_dev = _rel(_logits(mine, ids), want)
    print(f"relative L2 deviation of the logits: reference's rotated weights {ref_dev:.3e}, ours {my_dev:.3e}")
    assert 0 < ref_dev < 1e-2  # fp16 weight rounding, not a different function
    assert my_dev <= 2 * ref_dev
    # the stages matter: without the norm fused, or with only one side of v / o turned, the function is another one
    assert _rel(_logits(R.rotate_ov(R.rotate_q(fx.orig, HIDDEN, fx.signs), HEAD_DIM), ids), want) > 20 * ref_dev
    half = dict(mine)
    half["model.layers.0.self_attn.o_proj.weight"] = fx.rotq["model.layers.0.self_attn.o_proj.weight"]
    assert _rel(_logits(half, ids), want) > 20 * ref_dev

    # tied embeddings: the embedding is rotated ONCE and keeps no norm; the new lm_head is the embedding with the final norm, rotated
    tied = {k: v for k, v in fx.orig.items() if k != "lm_head.weight"}
    want_t = _logits(tied, ids)
    mine_t = R.rotate_model(tied, HIDDEN, HEAD_DIM, fx.signs, tied=True)
    embed = tied["model.embed_tokens.weight"]
    assert _same(mine_t["model.embed_tokens.weight"], R.hadamard_rows(embed, HIDDEN, fx.signs))
    head = R.to_dtype(embed.astype(np.float64) * fx.orig["model.norm.weight"].astype(np.float64), np.float16)
    assert _same(mine_t["lm_head.weight"], R.hadamard_rows(head, HIDDEN, fx.signs))
    dev_t = _rel(_logits(mine_t, ids), want_t)
    print(f"tied: {dev_t:.3e}")
    assert dev_t <= 2 * ref_dev


def test_torch_fuse_step_is_the_restatement(fx):
    from qqq_amd.quant import fuse_layer_norms, hadamard_matrix, hadamard_signs

    cfg = SimpleNamespace(**CONFIG)
    sd = {k: torch.from_numpy(v.copy()) for k, v in fx.orig.items()}
    before = {k: v.clone() for k, v in sd.items()}
    got = fuse_layer_norms(sd, cfg)
    assert all(torch.equal(sd[k], before[k]) for k in sd)  # nothing in place
    for k, v in fx.fused.items():
        assert _same(got[k].numpy(), v), k
    # tied, by the config or by a missing lm_head: an lm_head of its own, the embedding as it was
    tied = {k: v for k, v in sd.items() if k != "lm_head.weight"}
    want = R.fuse_layer_norms({k: v.numpy() for k, v in tied.items()}, tied=True)
    for src, c in ((tied, cfg), (dict(sd, **{"lm_head.weight": sd["model.embed_tokens.weight"]}), SimpleNamespace(**dict(CONFIG, tie_word_embeddings=True)))):
        got = fuse_layer_norms(src, c)
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert _same(got[k].numpy(), v), k
        assert got["lm_head.weight"].data_ptr() != got["model.embed_tokens.weight"].data_ptr()
        assert torch.equal(got["model.embed_tokens.weight"], sd["model.embed_tokens.weight"])
    # f32 state dicts pass, bf16 is refused by name
    f32 = fuse_layer_norms({k: v.float() for k, v in sd.items()}, cfg)
    assert f32["lm_head.weight"].dtype == torch.float32
    with pytest.raises(RuntimeError, match="fuse_layer_norms: .* is bfloat16"):
        fuse_layer_norms({k: v.bfloat16() for k, v in sd.items()}, cfg)
    # the signs and the matrix they stand for
    s = hadamard_signs(64, torch.Generator().manual_seed(1))
    assert s.dtype == torch.int8 and s.shape == (64,) and set(s.tolist()) == {-1, 1}
    assert torch.equal(s, hadamard_signs(64, torch.Generator().manual_seed(1)))
    assert _same(hadamard_matrix(torch.from_numpy(fx.signs)).numpy(), fx.g["Q"])


def test_rotation_refuses_what_it_cannot_do(fx):
    from qqq_amd.quant import ops, quantize_model, rotate_model, rotate_state_dict

    sd = {k: torch.from_numpy(v.copy()) for k, v in fx.fused.items()}
    cfg = SimpleNamespace(**CONFIG)
    odd = SimpleNamespace(**dict(CONFIG, hidden_size=96, num_attention_heads=6))
    with pytest.raises(RuntimeError, match="rotate_state_dict: hidden_size = 96 is not a power of two.*Paley.*mode='random'"):
        rotate_state_dict(sd, odd)
    with pytest.raises(RuntimeError, match="rotate_state_dict: head_dim = 24"):
        rotate_state_dict(sd, SimpleNamespace(**dict(CONFIG, hidden_size=96, num_attention_heads=4)))
    with pytest.raises(RuntimeError, match="rotate_state_dict: mode"):
        rotate_state_dict(sd, cfg, mode="paley")
    with pytest.raises(RuntimeError, match="rotate_state_dict: signs belong"):
        rotate_state_dict(sd, cfg, mode="random", signs=torch.ones(64, dtype=torch.int8))
    with pytest.raises(RuntimeError, match="rotate_state_dict: Q must be a float64"):
        rotate_state_dict(sd, cfg, Q=torch.eye(64))
    with pytest.raises(RuntimeError, match="rotate_state_dict: the state dict has no lm_head.weight"):
        rotate_state_dict({k: v for k, v in sd.items() if k != "lm_head.weight"}, cfg)
    bad = torch.ones(64, dtype=torch.int8)
    bad[3] = 0
    with pytest.raises(RuntimeError, match="rotate_state_dict: every entry of sign must be"):
        rotate_state_dict(sd, cfg, signs=bad)
    with pytest.raises(RuntimeError, match="rotate_state_dict: sign must be contiguous int8 \\[64\\]"):
        rotate_state_dict(sd, cfg, signs=torch.ones(32, dtype=torch.int8))
    with pytest.raises(RuntimeError, match="is bfloat16"):
        rotate_model({k: torch.from_numpy(v.copy()).bfloat16() for k, v in fx.orig.items()}, cfg)
    with pytest.raises(RuntimeError, match="quantize_model: rotation must be"):
        quantize_model(sd, cfg, torch.zeros((1, 8), dtype=torch.int64), -1, rotation=3)
    # the op's wrapper checks views before anything reaches the library
    x = torch.zeros((4, 64), dtype=torch.float16)
    for kw, msg in ((dict(x=x.double(), n=64), "hadamard_rows: x must be a float16 or float32 matrix"),
                    (dict(x=x[0], n=64), "hadamard_rows: x must be a float16 or float32 matrix"),
                    (dict(x=x, n=48), "hadamard_rows: n must be a power of two"),
                    (dict(x=x, n=1), "hadamard_rows: n must be a power of two"),
                    (dict(x=x, n=16384), "hadamard_rows: n must be a power of two"),
                    (dict(x=x, n=128), "hadamard_rows: x has 64 columns, no multiple of n = 128"),
                    (dict(x=x.t(), n=4), "unit column stride"),
                    (dict(x=x, n=64, out=torch.zeros((4, 64))), "hadamard_rows: out must be a float16 matrix"),
                    (dict(x=x, n=64, out=torch.zeros((4, 32), dtype=torch.float16)), "hadamard_rows: out has the shape"),
                    (dict(x=x, n=64, sign=torch.ones(64)), "hadamard_rows: sign must be contiguous int8 \\[64\\]"),
                    (dict(x=x, n=64, sign=torch.ones(32, dtype=torch.int8)), "hadamard_rows: sign must be contiguous int8 \\[64\\]"),
                    (dict(x=x, n=64), "hadamard_rows: every tensor must be on the GPU")):
        with pytest.raises(RuntimeError, match=msg):
            ops.hadamard_rows(**kw)
    with pytest.raises(RuntimeError, match="check_signs: every entry"):
        ops.check_signs(torch.zeros(8, dtype=torch.int8), 8)
    assert ops.check_signs(torch.tensor([1, -1], dtype=torch.int8), 2) is not None


def test_rotate_header_binds_beside_the_quantisers():
    from qqq_amd import _abi, build
    from qqq_amd.quant import _lib as qlib

    L = qlib.lib()
    header = os.path.join(build.QUANT_INCLUDE, "qqq_amd_rotate.h")
    protos = _abi.prototypes(header)
    assert set(protos) == {"qqq_hadamard_rows"}
    ret, params = protos["qqq_hadamard_rows"]
    assert ret == "int" and len(params) == 11 and len(L.qqq_hadamard_rows.argtypes) == 11
    assert all(_abi.ctype_of(p) in (ctypes.c_void_p, ctypes.c_int) for p in params)
    # a header of its own, beside the quantiser's and outside include/: the pinned ABI of the first stays what it was
    assert header in build.quant_headers() and os.path.dirname(header) == os.path.dirname(build.QUANT_HEADER)
    assert "qqq_hadamard_rows" not in _abi.prototypes(build.QUANT_HEADER) and L.qqq_quant_abi_version() == 1


def test_entry_point_refuses_bad_arguments_by_name():
    from qqq_amd.quant import _lib as qlib

    L = qlib.lib()
    buf = (ctypes.c_float * 1024)()
    p = ctypes.addressof(buf)
    q = p + 2048
    ok = dict(X=p, ldx=128, Y=q, ldy=128, rows=2, cols=128, n=64, sign=None, dtype=0)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.qqq_hadamard_rows(a["X"], a["ldx"], a["Y"], a["ldy"], a["rows"], a["cols"], a["n"], a["sign"], a["dtype"], 0, None)
        return rc, qlib.last_error()

    for kw in (dict(dtype=2), dict(dtype=-1), dict(n=0), dict(n=1), dict(n=48), dict(n=16384), dict(n=-64), dict(rows=0), dict(cols=0),
               dict(cols=96), dict(cols=32), dict(ldx=127), dict(ldy=64), dict(X=None), dict(Y=None), dict(X=p + 1), dict(Y=q + 1),
               dict(dtype=1, X=p + 2), dict(Y=p, ldy=256, ldx=128), dict(Y=p + 64), dict(Y=p + 2 * 130), dict(X=q, Y=p + 2048 - 2 * 100)):
        rc, msg = call(**kw)
        assert rc == qlib.ERR_ARG and msg.startswith("qqq_hadamard_rows: "), (kw, rc, msg)
