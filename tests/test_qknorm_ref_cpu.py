"""Qwen3 support without a GPU: the numpy restatement of the fused q / k norm (tests/qknorm_ref.py) against transformers' Qwen3RMSNorm and
apply_rotary_pos_emb in fp16 on the CPU, the C header's rules, the recorded Qwen3 state-dict names (tests/golden/qwen3_state_dict.json)
against QuantLlamaForCausalLM.from_config, and from_config's routing.

The norm's tolerance: both sides compute fp16(w * fp16(x * r)) with r an f32 value of rsqrt(mean(x^2) + eps).  The restatement's r is the
correctly rounded f32 of the f64 mean; torch's comes from an f32 mean (relative error up to about d * 2^-24 in the worst summation order,
in practice a few 2^-24) and an rsqrt of its own.  r differs by a few f32 ulps at the most, which moves x * r across an fp16 rounding
boundary for about 2^-13 * (a few) of the elements, by one fp16 ulp; the second rounding (times w) can turn one ulp of n into two of y where
|w| mantissa is large.  So: at most 2 fp16 ulps anywhere, and at most 1 element in 1000 differing at all."""
import json
import os
import types

import numpy as np
import pytest
import torch

import act_ref
import qknorm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_ops", "qqq_amd_qknorm.h")
ENTRY_POINTS = ("qqq_rope_qkv_norm", "qqq_rope_qkv_norm_kv8", "qqq_rope_qkv_norm_paged", "qqq_rope_qkv_norm_paged_kv8")
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "qwen3_state_dict.json")))
EPS = 1e-6


def _config(**over):
    c = dict(FIXTURE["config"])
    c.update(over)
    return types.SimpleNamespace(**c)


def _hf_norm(d, w):
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm

    n = Qwen3RMSNorm(d, eps=EPS).half()
    n.weight.data.copy_(w)
    return n


# ---- the restatement against transformers

@pytest.mark.parametrize("d", [64, 128])
def test_the_norm_stage_is_qwen3_rmsnorm_within_two_ulps(d):
    g = torch.Generator().manual_seed(d)
    w = (1 + 0.3 * torch.randn(d, generator=g)).half()
    hf = _hf_norm(d, w)
    for amp in (0.01, 1.0, 30.0):
        x = (torch.randn((20000, d), generator=g) * amp).half()
        with torch.no_grad():
            want = hf(x)
        got = torch.from_numpy(R.norm(x.numpy(), w.numpy(), EPS))
        ulps = act_ref.ulp_diff(got, want)
        differ = int((ulps != 0).sum())
        print(f"d={d} amp={amp}: {differ} of {x.numel()} elements differ ({differ / x.numel():.2e}), "
              f"{int((ulps == 2).sum())} by 2 ulps, max {int(ulps.max())}")
        assert int(ulps.max()) <= 2
        assert differ * 1000 <= x.numel()


@pytest.mark.parametrize("d", [64, 128])
def test_an_all_zero_row_gives_zeros(d):
    w = (1 + 0.3 * torch.randn(d, generator=torch.Generator().manual_seed(1))).half().numpy()
    x = np.zeros((3, d), np.float16)
    x[1] = 1.0
    y = R.norm(x, w, EPS)
    assert (y[0] == 0).all() and (y[2] == 0).all() and (y[1] != 0).all()
    assert (R.sumsq(x) == np.array([0.0, float(d), 0.0])).all()


def test_the_sum_of_squares_is_the_stated_order_and_lanes_agree():
    # magnitudes 2^80 apart: an f64 sum in another order rounds differently, and sumsq() itself asserts that every lane ends equal
    rng = np.random.default_rng(0)
    for d in (64, 128):
        x = (rng.standard_normal((500, d)) * np.exp2(rng.integers(-20, 14, (500, d)))).astype(np.float16)
        ss = R.sumsq(x)
        exact = np.array([float(sum(int(round(float(v) * 2.0 ** 24)) ** 2 for v in row)) for row in x]) / 2.0 ** 48  # integer arithmetic
        assert np.all(np.abs(ss - exact) <= np.abs(exact) * 2.0 ** -50)


@pytest.mark.parametrize("d", [64, 128])
def test_the_rope_stage_is_apply_rotary_pos_emb_bit_for_bit(d):
    from transformers.models.qwen3.modeling_qwen3 import apply_rotary_pos_emb

    g = torch.Generator().manual_seed(7 + d)
    b, s, h, kvh = 2, 9, 3, 1
    w = (1 + 0.3 * torch.randn(d, generator=g)).half()
    hf = _hf_norm(d, w)
    q = torch.randn((b, s, h, d), generator=g).half()
    k = (torch.randn((b, s, kvh, d), generator=g) * 4).half()
    cos, sin = (torch.rand((40, d), generator=g) * 2 - 1).half(), (torch.rand((40, d), generator=g) * 2 - 1).half()
    pos = torch.randint(0, 40, (b, s), generator=g)
    with torch.no_grad():
        qn, kn = hf(q).transpose(1, 2), hf(k).transpose(1, 2)  # [b, heads, s, d], as Qwen3Attention.forward forms them
        want_q, want_k = apply_rotary_pos_emb(qn, kn, cos[pos], sin[pos])
    for normed, want, heads in ((qn, want_q, h), (kn, want_k, kvh)):
        rows = normed.transpose(1, 2).reshape(b * s * heads, d).numpy()  # token-major head rows
        p = pos.reshape(-1).repeat_interleave(heads).numpy()
        got = R.rope(rows, cos.numpy()[p], sin.numpy()[p])
        want_rows = want.transpose(1, 2).reshape(b * s * heads, d).numpy()
        assert np.array_equal(got.view(np.uint16), want_rows.view(np.uint16))


# ---- the header

def test_the_entry_points_are_declared_in_their_own_header_and_nowhere_else():
    from qqq_amd import _abi, _lib
    from qqq_amd import build as kb

    protos = _abi.prototypes(HEADER)
    assert tuple(protos) == ENTRY_POINTS
    assert kb.OPS_INCLUDE == os.path.join(ROOT, "include_ops") and HEADER in kb.operator_op_headers() and HEADER not in kb.headers()
    assert [d for d in os.listdir(kb.OPS_INCLUDE) if os.path.isdir(os.path.join(kb.OPS_INCLUDE, d))] == []  # flat, like include/
    for other in kb.headers() + kb.operator_op_headers():
        if other != HEADER:
            assert not set(ENTRY_POINTS) & set(_abi.prototypes(other)), other
    lib = _lib.lib()  # bound from the header like every other entry point
    for name, (_, params) in protos.items():
        assert len(getattr(lib, name).argtypes) == len(params), name
    allowed = {"const void*", "void*", "int", "float", "size_t"}
    for name, (ret, params) in protos.items():
        assert ret == "int"
        assert {_abi._spelling(p.rsplit(" ", 1)[0]) for p in params} <= allowed, name
    # each takes its counterpart's list with q_weight, k_weight, eps after ld_v
    names = lambda ps: [p.rsplit(" ", 1)[1].lstrip("*") for p in ps]
    for name, base_header in (("qqq_rope_qkv", "qqq_amd_attn.h"), ("qqq_rope_qkv_kv8", "qqq_amd_kv8.h"), ("qqq_rope_qkv_paged", "qqq_amd_paged.h"),
                              ("qqq_rope_qkv_paged_kv8", "qqq_amd_paged.h")):
        base = _abi.prototypes(kb.header(base_header))[name][1]
        new = protos[name.replace("qqq_rope_qkv", "qqq_rope_qkv_norm")][1]
        i = names(base).index("ld_v") + 1
        assert [" ".join(p.split()) for p in new] == [" ".join(p.split()) for p in base[:i]] + \
            ["const void* q_weight", "const void* k_weight", "float eps"] + [" ".join(p.split()) for p in base[i:]]
    unit = open(kb.SRC).read()
    assert '#include "qqq_qknorm.hip.h"' in unit and '#include "../../include_ops/qqq_amd_qknorm.h"' in unit
    assert _lib.ABI_VERSION == 4


def test_a_newer_qknorm_header_rebuilds_the_operator_library(monkeypatch):
    from qqq_amd import build as kb

    kb.build()
    assert not kb.needs_build()
    real = os.path.getmtime
    monkeypatch.setattr(os.path, "getmtime", lambda p: real(kb.LIB) + 10 if p == HEADER else real(p))
    assert kb.needs_build()


# ---- the model's state dict and from_config

def test_the_fixture_is_what_its_generator_writes():
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_qwen3_state_dict", os.path.join(ROOT, "tests", "golden", "gen_qwen3_state_dict.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.build() == FIXTURE


def _is_linear(key):
    return key.rsplit(".", 2)[-2].endswith("_proj")


def test_a_qwen3_config_exposes_transformers_names_and_loads_them_strictly():
    from qqq_amd import QuantLlamaForCausalLM, QuantLinear

    cfg = _config()
    m = QuantLlamaForCausalLM.from_config(cfg, 128)
    ours = m.state_dict()
    floats = {k: e for k, e in FIXTURE["entries"].items() if not _is_linear(k)}
    assert any(k.endswith("self_attn.q_norm.weight") for k in floats) and any(k.endswith("self_attn.k_norm.weight") for k in floats)
    got = {k: dict(shape=list(v.shape), dtype=str(v.dtype).replace("torch.", "")) for k, v in ours.items() if not _is_linear(k)}
    assert got == floats
    # the linears: transformers' <name>.weight [n, k] becomes the packed buffers of a QuantLinear(k, n), no bias (attention_bias is False)
    linears = {k[:-len(".weight")]: e["shape"] for k, e in FIXTURE["entries"].items() if _is_linear(k)}
    assert all(k.endswith(".weight") for k in FIXTURE["entries"] if _is_linear(k))
    packed = {k for k in ours if _is_linear(k)}
    assert packed == {f"{p}.{b}" for p in linears for b in ("B", "s_channel", "s_group")}
    for p, (n, k) in linears.items():
        mod = m.get_submodule(p)
        assert isinstance(mod, QuantLinear) and tuple(ours[p + ".B"].shape) == (k // 16, n * 2) and tuple(ours[p + ".s_channel"].shape) == (1, n)
    # head_dim comes from the config, not from hidden / heads
    a = m.model.layers[0].self_attn
    assert a.head_dim == 128 and a.qk_norm and a.q_norm.eps == cfg.rms_norm_eps
    assert bool((a.q_norm.weight == 1).all()) and a.q_norm.weight.dtype == torch.float16 and not a.q_norm.weight.requires_grad
    # strict load, tied
    assert m.lm_head.weight is m.model.embed_tokens.weight
    dt = {"float16": torch.float16}
    sd = {k: torch.full(e["shape"], 0.5, dtype=dt[e["dtype"]]) for k, e in floats.items()}
    sd.update({k: v.clone() for k, v in ours.items() if _is_linear(k)})
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert m.lm_head.weight is m.model.embed_tokens.weight
    assert bool((a.k_norm.weight == 0.5).all())


def test_from_config_routes_qwen3_and_leaves_llama_and_qwen2_without_norms():
    from qqq_amd import QuantLlamaAttention, QuantLlamaForCausalLM

    with pytest.raises(NotImplementedError, match="sliding-window"):
        QuantLlamaForCausalLM.from_config(_config(use_sliding_window=True), 128)
    with pytest.raises(NotImplementedError, match="layer_types"):
        QuantLlamaForCausalLM.from_config(_config(layer_types=["full_attention", "sliding_attention"]), 128)
    with torch.device("meta"):
        untied = QuantLlamaForCausalLM.from_config(_config(tie_word_embeddings=False), 128)
        biased = QuantLlamaForCausalLM.from_config(_config(attention_bias=True), 128)
    assert untied.lm_head.weight is not untied.model.embed_tokens.weight
    sd = biased.state_dict()
    assert all(f"model.layers.0.self_attn.{n}_proj.bias" in sd for n in "qkvo")
    old = json.load(open(os.path.join(ROOT, "tests", "golden", "causal_lm_state_dict.json")))
    for name in ("llama", "qwen2"):
        c = {k: v for k, v in old[name]["config"].items() if k != "group_size"}
        with torch.device("meta"):
            lm = QuantLlamaForCausalLM.from_config(types.SimpleNamespace(**c), old[name]["config"]["group_size"])
        for layer in lm.model.layers:
            assert not layer.self_attn.qk_norm and not hasattr(layer.self_attn, "q_norm") and not hasattr(layer.self_attn, "k_norm")
        assert not any("q_norm" in k or "k_norm" in k for k in lm.state_dict())
    with pytest.raises(ValueError, match="head_dim"):
        QuantLlamaAttention(256, 8, 8, -1, head_dim=32, qk_norm=True)
    with torch.device("meta"):
        QuantLlamaAttention(256, 8, 8, -1, head_dim=32)  # without the norm the head size is as free as before


def test_the_ops_reject_what_the_kernel_does_not_take():
    from qqq_amd import ops

    d, h, kvh, m = 64, 2, 1, 3
    z = lambda *s, dt=torch.float16: torch.zeros(s, dtype=dt)
    q, k, v, cos, sin = z(m, h * d), z(m, kvh * d), z(m, kvh * d), z(8, d), z(8, d)
    pos, slots = z(m, dt=torch.int64), z(m, dt=torch.int64)
    kc, kp = z(1, kvh, 8, d), z(2, kvh, 16, d)
    w = torch.ones(d, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="rope_qkv_norm: .*GPU"):
        ops.rope_qkv_norm(q, k, v, w, w, EPS, cos, sin, pos, kc, kc.clone())
    with pytest.raises(RuntimeError, match="rope_qkv_norm_paged: .*GPU"):
        ops.rope_qkv_norm_paged(q, k, v, w, w, EPS, cos, sin, pos, slots, kp, kp.clone())
