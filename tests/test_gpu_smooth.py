"""The smoothing search on the GPU against the CPU restatement (tests/smooth_ref.py) on the inputs recorded with the reference's own
classes (tests/golden/smooth_small.npz): the candidate walk, every candidate's loss, the chosen range, fused against composed; then
smooth_scales and quantize_model(smooth=...) on a 2-layer model, per-channel and g128."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import smooth_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(kind, group) for kind in R.KINDS for group in (0, 128)]
# The largest relative deviation of a device loss from the restatement's CPU loss on this fixture, measured on an MI355X: 8.1e-4 (qkv
# per-channel; 6.6e-4 qkv g128, 2.2e-4 with 2 KV heads, 1.1e-5 ... 3.2e-5 for the three plain linears).  The fp16 GEMMs sum in another
# order; the fake-quantised operands are bit-identical.  Times four: headroom for another GEMM kernel choice.  Whatever is measured
# later, the test refuses an EPS above 1e-2.
MEASURED = 8.1e-4
EPS = 4 * MEASURED


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "smooth_small.npz"))


@pytest.fixture(scope="module")
def searched(g, dev):
    """per case: the restatement's CPU search and the device's, fused and composed, each run once"""
    from qqq_amd.quant.smooth import migration_scale

    out = {}
    for kind, group in CASES:
        x, w, mk, extra, _ = R.golden_case(g, kind, group)
        cpu = R.search_os(x, w, mk, group, extra)
        ex = None if extra is None else {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in extra.items()}
        fused, composed = {}, {}
        s_f = migration_scale(x.to(dev), w.to(dev), mk, group or -1, "os+", ex, fused=True, trace=fused)
        s_c = migration_scale(x.to(dev), w.to(dev), mk, group or -1, "os+", ex, fused=False, trace=composed)
        out[kind, group] = SimpleNamespace(cpu=cpu, s_f=s_f.cpu(), s_c=s_c.cpu(), fused=fused, composed=composed)
    return out


@pytest.mark.parametrize("kind,group", CASES)
def test_search_on_the_device_against_the_restatement(searched, kind, group):
    """MEASURED above (8.1e-4) is the largest `deviation` this test printed over all ten cases on an MI355X; in every case the device's
    chosen candidate was the CPU restatement's (and the reference's recorded one), fused and composed alike."""
    r = searched[kind, group]
    scale, ranges, losses, best = r.cpu
    assert r.fused["ranges"] == ranges and r.composed["ranges"] == ranges and len(ranges) >= 100
    cpu = np.array(losses, dtype=np.float64)
    dev_f, dev_c = np.array(r.fused["losses"]), np.array(r.composed["losses"])
    deviation = max(np.max(np.abs(dev_f - cpu) / cpu), np.max(np.abs(dev_c - cpu) / cpu))
    print(f"{kind} group {group}: deviation {deviation:.3e}, cpu best {best}, fused best {r.fused['best']}, composed best {r.composed['best']}")
    assert EPS <= 1e-2
    assert deviation <= EPS
    for tr in (r.fused, r.composed):  # the device's choice is as good as the CPU's, within what the GEMMs can move a loss by
        assert cpu[tr["best"]] <= (1 + EPS) / (1 - EPS) * cpu.min()
    assert torch.equal(r.s_f, r.s_c) and r.fused["best"] == r.composed["best"]
    assert r.s_f.dtype == torch.float16 and bool(torch.isfinite(r.s_f).all()) and float(r.s_f.min()) >= 1.0


def test_awq_and_sq_on_the_device(g, dev):
    from qqq_amd.quant.smooth import migration_scale

    x, w, mk, extra, _ = R.golden_case(g, "o_proj", 0)
    for group in (0, 128):
        tf, tc = {}, {}
        s_f = migration_scale(x.to(dev), w.to(dev), mk, group or -1, "awq", None, fused=True, trace=tf)
        s_c = migration_scale(x.to(dev), w.to(dev), mk, group or -1, "awq", None, fused=False, trace=tc)
        assert torch.equal(s_f, s_c) and tf["best"] == tc["best"] and len(tf["losses"]) == 20
        _, _, losses, best = R.search_awq(x, w, mk, group, None)
        assert np.allclose(tf["losses"], losses, rtol=1e-2, atol=0)
        assert losses[tf["best"]] <= 1.02 * min(losses)
    x, w, _, _, _ = R.golden_case(g, "down_proj", 0)
    s = migration_scale(x.to(dev), w.to(dev), "down_proj", -1, "sq").cpu()
    ref = R.search_sq(x, w)
    assert s.dtype == torch.float16 and bool(((s.float() - ref.float()).abs() <= 2.0 ** -10 * ref.float()).all())  # pow and sqrt may differ by an ulp


CONFIG = dict(model_type="llama", vocab_size=1000, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
              num_hidden_layers=2, rms_norm_eps=1e-6, rope_theta=10000.0)


def _model(seed=33):
    gen = torch.Generator().manual_seed(seed)
    h, inter, v, kv = 256, 512, 1000, 128
    emb = torch.randn((v, h), generator=gen)
    emb[:, 7] *= 12  # two outlier channels of the residual stream
    emb[:, 130] *= -9
    sd = {"model.embed_tokens.weight": emb.half(), "model.norm.weight": (1 + 0.1 * torch.randn(h, generator=gen)).half(),
          "lm_head.weight": (0.2 * torch.randn((v, h), generator=gen)).half()}
    shapes = {"self_attn.q_proj": (h, h), "self_attn.k_proj": (kv, h), "self_attn.v_proj": (kv, h), "self_attn.o_proj": (h, h),
              "mlp.gate_proj": (inter, h), "mlp.up_proj": (inter, h), "mlp.down_proj": (h, inter)}
    for i in range(2):
        for name, (n, k) in shapes.items():
            sd[f"model.layers.{i}.{name}.weight"] = (torch.randn((n, k), generator=gen) * k ** -0.5).half()
        for name in ("input_layernorm", "post_attention_layernorm"):
            sd[f"model.layers.{i}.{name}.weight"] = (1 + 0.1 * torch.randn(h, generator=gen)).half()
    return sd, torch.randint(0, v, (12, 64), generator=gen)


@pytest.mark.parametrize("gs", [-1, 128])
def test_smooth_scales_and_quantize_model(dev, gs):
    from qqq_amd.quant import quantize_model
    from qqq_amd.quant.smooth import apply_smooth, smooth_scales

    sd, ids = _model()
    cfg = SimpleNamespace(**CONFIG)
    scales = smooth_scales(sd, cfg, ids, gs, device=dev)
    assert len(scales) == 8 and [s.numel() for s in scales] == [256, 256, 256, 512] * 2
    for s in scales:
        assert s.dtype == torch.float16 and bool(torch.isfinite(s).all()) and float(s.min()) >= 1.0
    assert float(scales[0].max()) > 1.0  # the outlier channels were found
    assert all(torch.equal(a, b) for a, b in zip(scales, smooth_scales(sd, cfg, ids[:8], gs, device=dev)))  # the first 8 sequences alone
    res = {}
    lm = quantize_model(sd, cfg, ids, gs, device=dev, results=res, smooth="os+")
    assert len(res["smooth"]) == 8 and all(torch.equal(a, b) for a, b in zip(res["smooth"], scales))
    again = quantize_model(sd, cfg, ids, gs, device=dev, smooth=[s.cpu() for s in scales])
    a, b = lm.state_dict(), again.state_dict()
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    prompts = [ids[0, :5].tolist(), ids[1, :17].tolist()]
    toks = lm.generate(prompts, 4)
    assert toks == again.generate(prompts, 4) and all(len(t) == 4 and all(0 <= x < 1000 for x in t) for t in toks)
    # the norms carry 1 / s, GQA leaves o_proj's scale out of the checkpoint
    smoothed = apply_smooth(sd, cfg, scales)
    assert torch.equal(a["model.layers.0.input_layernorm.weight"].cpu(), smoothed["model.layers.0.input_layernorm.weight"])
    plain = quantize_model(sd, cfg, ids, gs, device=dev)
    assert not torch.equal(plain.state_dict()["model.layers.0.input_layernorm.weight"], a["model.layers.0.input_layernorm.weight"])
