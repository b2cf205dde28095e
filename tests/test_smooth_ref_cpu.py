"""Smoothing without a GPU: the CPU restatement (tests/smooth_ref.py) and the package's own search with the torch-composed
fake-quantisation (fused=False) against the fixture recorded from the reference's own migration classes (tests/golden/smooth_small.npz,
gen_smooth_golden.py); apply_smooth against literal per-tensor expectations and, in f64, the invariance of every folded pair; the new
header's place in the quantiser's library."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import smooth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(kind, group) for kind in R.KINDS for group in (0, 128)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _same(a, b):
    return a.dtype == b.dtype == np.float16 and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "smooth_small.npz"))


@pytest.fixture(scope="module")
def searched(g):
    """the restatement's os+ search of every case, computed once: (scale, ranges, losses, best)"""
    out = {}
    for kind, group in CASES:
        x, w, mk, extra, _ = R.golden_case(g, kind, group)
        out[kind, group] = R.search_os(x, w, mk, group, extra)
    return out


@pytest.mark.parametrize("kind,group", CASES)
def test_restatement_search_matches_the_reference(g, searched, kind, group):
    _, _, _, _, rec = R.golden_case(g, kind, group)
    scale, ranges, losses, best = searched[kind, group]
    assert len(ranges) == int(rec["count"]) >= 100 and np.array_equal(np.array(ranges), rec["ranges"])
    rel = np.abs(np.array(losses, dtype=np.float64) - rec["losses"]) / rec["losses"]
    print(kind, group, "largest relative loss difference", rel.max(), "bound", float(rec["loss_bound"]))
    assert rel.max() <= float(rec["loss_bound"])
    assert best == int(rec["best"]) and _same(scale.numpy(), rec["scale"])
    assert float(scale.min()) >= 1.0 and float(scale.max()) > 1.0  # os+ only ever scales outliers down


@pytest.mark.parametrize("kind,group", CASES)
def test_restatement_fake_quant_matches_the_reference(g, kind, group):
    x, w, mk, extra, rec = R.golden_case(g, kind, group)
    for n, i in enumerate(rec["at"]):
        _, qx, qw = R.os_loss(x, w, mk, group, float(rec["ranges"][i]), extra, tgt=torch.zeros(1))
        assert _same(qx.numpy().reshape(x.shape), rec["qx"][n])
        assert _same(qw.numpy()[rec["qw_rows"]], rec["qw"][n])
        assert not (_bits(qx.numpy()) == 0x8000).any() and not (_bits(qw.numpy()) == 0x8000).any()


def test_restatement_awq_and_sq_match_the_reference(g):
    x, w, mk, extra, _ = R.golden_case(g, "o_proj", 0)
    for group in (0, 128):
        tag = f"awq_o_proj_{'g128' if group else 'pc'}"
        scale, ratios, losses, best = R.search_awq(x, w, mk, group, extra)
        assert ratios == [c / 20 for c in range(20)] and best == int(g[tag + "/best"])
        assert _same(scale.numpy(), g[tag + "/scale"])
        assert np.allclose(losses, g[tag + "/losses"], rtol=1e-3, atol=0)
    x, w, _, _, _ = R.golden_case(g, "down_proj", 0)
    assert _same(R.search_sq(x, w).numpy(), g["sq_down_proj/scale"])


def _cases(rng):
    for rows, cols, group in ((1, 8, 0), (3, 136, 0), (5, 2056, 0), (3, 128, 128), (4, 384, 128)):
        x = (rng.standard_normal((rows, cols)) * 3).astype(np.float16)
        x[0] = 0  # an all-zero row
        if rows > 2:
            x[1] = (rng.standard_normal(cols) * 1e-6).astype(np.float16)  # the eps clamp
            x[2, : cols // 2] = (np.arange(cols // 2) % 16 + 0.5).astype(np.float16)  # ties, once the scale is 1
            x[2, cols // 2] = 127
        c = np.where(rng.random(cols) < 0.25, rng.random(cols) * 6 + 1, 1).astype(np.float16)
        yield x, c, group


def test_torch_composition_has_the_restatements_bits():
    """fake_quant_torch (fused=False) is the reference's sequence of torch calls; the numpy restatement states one rounding per line"""
    from qqq_amd.quant.smooth import fake_quant_torch

    rng = np.random.default_rng(3)
    for x, c, group in _cases(rng):
        for bits in (8, 4):
            for divide in (True, False):
                for cs in (None, c):
                    ref = R.fake_quant_rows(x, cs, bits, group, divide)
                    got = fake_quant_torch(torch.from_numpy(x), None if cs is None else torch.from_numpy(cs), bits, group, divide).numpy()
                    assert _same(got, ref), (x.shape, group, bits, divide, cs is None)
                    assert not (_bits(ref) == 0x8000).any()
                    assert not ref[0].any()
    # exact .5 ties round to even: scale 1 (row maximum 127 at 8 bits), 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    x = np.zeros((1, 8), np.float16)
    x[0] = [127, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5]
    assert R.fake_quant_rows(x, None, 8).tolist() == [[127, 0, 2, 2, 0, -2, -2, 4]]


@pytest.mark.parametrize("kind,group", [("qkv_gqa", 0), ("o_proj", 128), ("up_and_gate", 0), ("down_proj", 128)])
def test_package_search_composed_matches_the_reference(g, kind, group):
    """migration_scale(fused=False) on the CPU: the package's walk, scale formula and module functions against the reference's record"""
    from qqq_amd.quant.smooth import migration_scale

    x, w, mk, extra, rec = R.golden_case(g, kind, group)
    trace = {}
    scale = migration_scale(x, w, mk, group or -1, "os+", extra, fused=False, trace=trace)
    assert trace["ranges"] == rec["ranges"].tolist() and trace["best"] == int(rec["best"])
    assert np.max(np.abs(np.array(trace["losses"]) - rec["losses"]) / rec["losses"]) <= float(rec["loss_bound"])
    assert _same(scale.numpy(), rec["scale"])


def test_package_awq_and_sq_composed_match_the_reference(g):
    from qqq_amd.quant.smooth import migration_scale

    x, w, mk, extra, _ = R.golden_case(g, "o_proj", 0)
    for group in (0, 128):
        tag = f"awq_o_proj_{'g128' if group else 'pc'}"
        trace = {}
        scale = migration_scale(x, w, mk, group or -1, "awq", extra, fused=False, trace=trace)
        assert trace["best"] == int(g[tag + "/best"]) and _same(scale.numpy(), g[tag + "/scale"])
    x, w, _, _, _ = R.golden_case(g, "down_proj", 0)
    assert _same(migration_scale(x, w, "down_proj", -1, "sq", fused=False).numpy(), g["sq_down_proj/scale"])
    for bad in (dict(kind="k_proj"), dict(method="os"), dict(group_size=64)):
        kw = dict(dict(kind="down_proj", group_size=-1, method="os+"), **bad)
        with pytest.raises(RuntimeError, match="migration_scale: "):
            migration_scale(x, w, fused=False, **kw)


HID, INTER = 16, 24


def _tiny(kv_heads, qwen):
    gen = torch.Generator().manual_seed(5)
    r = lambda *s: (torch.randn(*s, generator=gen) * 0.3).half()
    cfg = SimpleNamespace(model_type="qwen2" if qwen else "llama", hidden_size=HID, num_attention_heads=4, num_key_value_heads=kv_heads,
                          intermediate_size=INTER, num_hidden_layers=2, rms_norm_eps=1e-6, rope_theta=10000.0, vocab_size=32)
    sd = {"model.embed_tokens.weight": r(32, HID), "model.norm.weight": r(HID), "lm_head.weight": r(32, HID)}
    for i in range(2):
        p = f"model.layers.{i}."
        sd[p + "input_layernorm.weight"] = r(HID) + 1
        sd[p + "post_attention_layernorm.weight"] = r(HID) + 1
        for n, rows in (("q_proj", HID), ("k_proj", 4 * kv_heads), ("v_proj", 4 * kv_heads)):
            sd[p + f"self_attn.{n}.weight"] = r(rows, HID)
            if qwen:
                sd[p + f"self_attn.{n}.bias"] = r(rows)
        sd[p + "self_attn.o_proj.weight"] = r(HID, HID)
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"], sd[p + "mlp.down_proj.weight"] = r(INTER, HID), r(INTER, HID), r(HID, INTER)
    scales = []
    for i in range(2):
        scales += [(torch.rand(n, generator=gen) * 3 + 1).half() for n in (HID, HID, HID, INTER)]
    return cfg, sd, scales


@pytest.mark.parametrize("kv_heads,qwen", [(4, False), (4, True), (2, True)])
def test_apply_smooth_per_tensor(kv_heads, qwen):
    from qqq_amd.quant.smooth import apply_smooth

    cfg, sd, scales = _tiny(kv_heads, qwen)
    before = {k: v.clone() for k, v in sd.items()}
    out = apply_smooth(sd, cfg, scales)
    assert all(torch.equal(sd[k], before[k]) for k in sd) and set(out) == set(sd)  # a new dict, the input untouched
    mha = kv_heads == 4
    expect = dict(before)
    for i in range(2):
        p = f"model.layers.{i}."
        s_qkv, s_o, s_gu, s_d = scales[4 * i: 4 * i + 4]
        expect[p + "input_layernorm.weight"] = before[p + "input_layernorm.weight"] / s_qkv
        for n in ("q_proj", "k_proj"):
            expect[p + f"self_attn.{n}.weight"] = before[p + f"self_attn.{n}.weight"] * s_qkv
        v = before[p + "self_attn.v_proj.weight"] * s_qkv
        expect[p + "self_attn.v_proj.weight"] = v / s_o.reshape(-1, 1) if mha else v
        expect[p + "self_attn.o_proj.weight"] = before[p + "self_attn.o_proj.weight"] * s_o if mha else before[p + "self_attn.o_proj.weight"]
        if qwen and mha:
            expect[p + "self_attn.v_proj.bias"] = before[p + "self_attn.v_proj.bias"] / s_o
        expect[p + "post_attention_layernorm.weight"] = before[p + "post_attention_layernorm.weight"] / s_gu
        expect[p + "mlp.gate_proj.weight"] = before[p + "mlp.gate_proj.weight"] * s_gu
        expect[p + "mlp.up_proj.weight"] = (before[p + "mlp.up_proj.weight"] * s_gu) / s_d.reshape(-1, 1)
        expect[p + "mlp.down_proj.weight"] = before[p + "mlp.down_proj.weight"] * s_d
    for k in sd:
        assert out[k].dtype == torch.float16 and torch.equal(out[k], expect[k]), k
    for k in ("self_attn.q_proj.bias", "self_attn.k_proj.bias"):
        if qwen:
            assert torch.equal(out["model.layers.0." + k], before["model.layers.0." + k])
    # every folded pair is unchanged within two fp16 roundings: |p' - p| <= 3 * 2^-11 |p|, in f64.  Where a tensor takes two scales
    # (v: s_qkv then 1 / s_o, up: s_gate_up then 1 / s_down) each pair is held against the tensor as its first scale left it.
    bound = 3 * 2.0 ** -11
    d = lambda t: t.double()
    for i in range(2):
        p = f"model.layers.{i}."
        s_qkv, s_o, s_gu, s_d = scales[4 * i: 4 * i + 4]
        ln1, ln2 = p + "input_layernorm.weight", p + "post_attention_layernorm.weight"
        pairs = [(d(before[ln1]) * d(before[p + f"self_attn.{n}.weight"]), d(out[ln1]) * d(out[p + f"self_attn.{n}.weight"])) for n in ("q_proj", "k_proj")]
        pairs += [(d(before[ln2]) * d(before[p + "mlp.gate_proj.weight"]), d(out[ln2]) * d(out[p + "mlp.gate_proj.weight"]))]
        # up rows . down columns: down[o, j] * up[j, c] for every (o, j, c)
        pairs += [(d(before[p + "mlp.down_proj.weight"])[:, :, None] * d(before[p + "mlp.up_proj.weight"] * s_gu)[None],
                   d(out[p + "mlp.down_proj.weight"])[:, :, None] * d(out[p + "mlp.up_proj.weight"])[None])]
        if mha:  # v rows . o columns: kv_heads == heads, column j of o reads row j of v
            pairs += [(d(before[p + "self_attn.o_proj.weight"])[:, :, None] * d(before[p + "self_attn.v_proj.weight"] * s_qkv)[None],
                       d(out[p + "self_attn.o_proj.weight"])[:, :, None] * d(out[p + "self_attn.v_proj.weight"])[None])]
            if qwen:
                pairs += [(d(before[p + "self_attn.o_proj.weight"]) * d(before[p + "self_attn.v_proj.bias"]),
                           d(out[p + "self_attn.o_proj.weight"]) * d(out[p + "self_attn.v_proj.bias"]))]
        else:  # the skip: v only took s_qkv, o is untouched
            pairs += [(d(before[ln1]) * d(before[p + "self_attn.v_proj.weight"]), d(out[ln1]) * d(out[p + "self_attn.v_proj.weight"]))]
        for a, b in pairs:
            assert bool(((b - a).abs() <= bound * a.abs()).all())


def test_apply_smooth_and_quantize_model_refusals():
    from qqq_amd.quant import quantize_model
    from qqq_amd.quant.smooth import apply_smooth

    cfg, sd, scales = _tiny(4, False)
    with pytest.raises(RuntimeError, match=r"apply_smooth: scale_list must hold 4 \* 2 vectors, got 7"):
        apply_smooth(sd, cfg, scales[:7])
    with pytest.raises(RuntimeError, match=r"apply_smooth: scale 1 must be float16 \[16\]"):
        apply_smooth(sd, cfg, [scales[0], scales[3]] + scales[2:])
    with pytest.raises(RuntimeError, match="is float32; smoothing is done in float16"):
        apply_smooth(dict(sd, **{"model.layers.0.mlp.down_proj.weight": sd["model.layers.0.mlp.down_proj.weight"].float()}), cfg, scales)
    for smooth in ("os", 3, {"a": 1}):
        with pytest.raises(RuntimeError, match="quantize_model: smooth must be None, one of"):
            quantize_model(sd, cfg, torch.zeros((1, 8), dtype=torch.int64), -1, smooth=smooth)


def test_fakequant_header_binds_beside_the_others():
    from qqq_amd import _abi, build
    from qqq_amd.quant import _lib as qlib

    L = qlib.lib()
    header = os.path.join(build.QUANT_OPS_INCLUDE, "qqq_amd_fakequant.h")
    assert build.QUANT_OPS_INCLUDE == os.path.join(ROOT, "qqq_amd", "quant", "include_ops")
    protos = _abi.prototypes(header)
    assert set(protos) == {"qqq_fake_quant_rows"}
    ret, params = protos["qqq_fake_quant_rows"]
    assert ret == "int" and len(params) == 12 and len(L.qqq_fake_quant_rows.argtypes) == 12
    assert all(_abi.ctype_of(p) in (ctypes.c_void_p, ctypes.c_int) for p in params)
    # membership, never a listing: the next quantiser op drops its header into the same directory
    assert header in build.quant_op_headers() and header not in build.quant_headers() + build.quant_ext_headers()
    seen = {}
    for h in build.quant_headers() + build.quant_ext_headers() + build.quant_op_headers():  # bound onto one handle: no name twice
        for name in _abi.prototypes(h):
            assert name not in seen, (name, seen[name], h)
            seen[name] = h
    assert "qqq_fake_quant_rows" not in _abi.prototypes(build.QUANT_HEADER) and L.qqq_quant_abi_version() == 1


def test_a_newer_fakequant_header_rebuilds_the_quantiser_library(monkeypatch):
    from qqq_amd import build

    build.build_quant()
    newer = os.path.join(build.QUANT_OPS_INCLUDE, "qqq_amd_fakequant.h")
    compiled = []
    monkeypatch.setattr(build, "_compile", lambda src, out, verbose, flags=(): compiled.append((src, out, tuple(flags))) or out)
    monkeypatch.setattr(os.path, "getmtime", lambda p: 2.0 if p == build.QUANT_LIB else 1.0)
    assert build.build_quant() == build.QUANT_LIB and not compiled
    monkeypatch.setattr(os.path, "getmtime", lambda p: 2.0 if p == build.QUANT_LIB else 3.0 if p == newer else 1.0)
    assert build.build_quant() == build.QUANT_LIB and compiled == [(build.QUANT_SRC, build.QUANT_LIB, build.QUANT_FLAGS)]


def test_entry_point_refuses_bad_arguments_by_name():
    from qqq_amd.quant import _lib as qlib

    L = qlib.lib()
    buf = (ctypes.c_uint16 * 8192)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    q = p + 4096
    ok = dict(X=p, ldx=256, Y=q, ldy=256, rows=4, cols=256, col_scale=None, bits=8, group=0, divide=0)
    order = ("X", "ldx", "Y", "ldy", "rows", "cols", "col_scale", "bits", "group", "divide")
    for bad, msg in ((dict(bits=6), "qqq_fake_quant_rows: bits=6 is not one of 4, 8"),
                     (dict(group=64), "qqq_fake_quant_rows: group=64 is not 0"),
                     (dict(divide=2), "qqq_fake_quant_rows: divide=2 must be 0 or 1"),
                     (dict(rows=0), "qqq_fake_quant_rows: bad shape rows=0"),
                     (dict(cols=12, ldx=16, ldy=16), "qqq_fake_quant_rows: bad shape rows=4 cols=12"),
                     (dict(cols=0), "qqq_fake_quant_rows: bad shape"),
                     (dict(ldx=248), "qqq_fake_quant_rows: bad shape"),
                     (dict(ldy=260), "qqq_fake_quant_rows: bad shape"),
                     (dict(cols=136, group=128), "qqq_fake_quant_rows: cols=136 is no multiple of group=128"),
                     (dict(X=None), "qqq_fake_quant_rows: bad argument"),
                     (dict(X=p + 8), "qqq_fake_quant_rows: bad argument"),
                     (dict(Y=q + 2), "qqq_fake_quant_rows: bad argument"),
                     (dict(col_scale=p + 4), "qqq_fake_quant_rows: bad argument"),
                     (dict(Y=p + 512), "qqq_fake_quant_rows: X and Y overlap"),
                     (dict(Y=p, ldy=512), "qqq_fake_quant_rows: X and Y overlap")):
        a = dict(ok, **bad)
        assert L.qqq_fake_quant_rows(*[a[k] for k in order], 0, None) == qlib.ERR_ARG, bad
        assert qlib.last_error().startswith(msg), (bad, qlib.last_error())
