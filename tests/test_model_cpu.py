"""QuantLlamaModel / QuantLlamaForCausalLM without a GPU: the state-dict against the recorded names of the reference's classes
(tests/golden/causal_lm_state_dict.json), weight tying, the refusals of from_config, the fuse_* forwarding, and generate()'s admission /
free bookkeeping with the forward pass and the sampler replaced by host stubs."""
import json
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "causal_lm_state_dict.json")))


def _config(name, **over):
    c = {k: v for k, v in FIXTURE[name]["config"].items() if k != "group_size"}
    c.update(over)
    return types.SimpleNamespace(**c), FIXTURE[name]["config"]["group_size"]


@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_state_dict_names_shapes_dtypes_are_the_reference_s(name):
    from qqq_amd import QuantLlamaForCausalLM

    cfg, gs = _config(name)
    with torch.device("meta"):
        m = QuantLlamaForCausalLM.from_config(cfg, gs)
    got = {k: dict(shape=list(v.shape), dtype=str(v.dtype).replace("torch.", "")) for k, v in m.state_dict().items()}
    assert got == FIXTURE[name]["entries"]
    assert len(m.model.layers) == cfg.num_hidden_layers and [l.self_attn.layer_idx for l in m.model.layers] == list(range(len(m.model.layers)))


def test_the_fixture_is_what_its_generator_writes():
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_causal_lm_state_dict", os.path.join(ROOT, "tests", "golden", "gen_causal_lm_state_dict.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for name, c in gen.CONFIGS.items():
        assert FIXTURE[name]["config"] == c
        assert FIXTURE[name]["entries"] == {k: dict(shape=s, dtype=t) for k, (s, t) in gen.entries(c).items()}


def test_a_reference_state_dict_loads_strictly_and_tying_shares_the_weight():
    from qqq_amd import QuantLlamaForCausalLM

    dt = {"float16": torch.float16, "float32": torch.float32, "int32": torch.int32}
    for name in FIXTURE:
        cfg, gs = _config(name)
        m = QuantLlamaForCausalLM.from_config(cfg, gs)
        tied = cfg.tie_word_embeddings
        assert (m.lm_head.weight is m.model.embed_tokens.weight) == tied
        sd = {k: torch.ones(e["shape"], dtype=dt[e["dtype"]]) for k, e in FIXTURE[name]["entries"].items()}
        res = m.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert (m.lm_head.weight is m.model.embed_tokens.weight) == tied
        assert m.lm_head.weight.dtype == torch.float16 and not m.lm_head.weight.requires_grad


def test_from_config_refusals_propagate_and_fuse_flags_reach_every_layer():
    from qqq_amd import QuantLlamaForCausalLM, QuantLlamaModel

    cfg, gs = _config("qwen2", use_sliding_window=True)
    with pytest.raises(NotImplementedError, match="sliding-window"):
        QuantLlamaForCausalLM.from_config(cfg, gs)
    cfg, gs = _config("llama", hidden_act="gelu")
    with pytest.raises(NotImplementedError, match="SiLU"):
        QuantLlamaModel.from_config(cfg, gs)
    cfg, gs = _config("llama", rope_scaling={"rope_type": "yarn", "factor": 2.0})
    with pytest.raises(NotImplementedError, match="rope_type"):
        QuantLlamaModel.from_config(cfg, gs)
    cfg, gs = _config("llama")
    with torch.device("meta"):
        m = QuantLlamaForCausalLM.from_config(cfg, gs)
    keys = sorted(m.state_dict())
    assert m.fuse_decode() is m and m.fuse_prefill() is m
    assert all(l.decode_fused and l.prefill_fused for l in m.model.layers)
    m.model.unfuse_decode().unfuse_prefill()
    assert not any(l.decode_fused or l.prefill_fused for l in m.model.layers)
    assert sorted(m.state_dict()) == keys


# ---- generate(): the bookkeeping, with host stubs for the forward pass and the sampler

class _Stub:
    """forward: logits whose argmax is (last token of the row's sequence + 1) % vocab; sampler: argmax.  Records every pass."""

    def __init__(self, m, monkeypatch):
        self.passes, self.m = [], m
        monkeypatch.setattr(m, "forward", self.forward)
        monkeypatch.setattr("qqq_amd.model.ops.sample_tokens", self.sample)

    def forward(self, ids, cache, step, all_rows=False):
        assert ids.dtype == torch.int64 and ids.shape == (sum(step.counts),)
        last = ids[step.cu_tokens[1:].long() - 1]
        self.passes.append(dict(counts=list(step.counts), starts=list(step.starts), free=cache.free_blocks, last=last.tolist()))
        return torch.nn.functional.one_hot((last + 1) % 50, 50).half()

    def sample(self, logits, T, k, p, u):
        assert u.shape == (logits.shape[0],) and u.dtype == torch.float32
        return logits.argmax(dim=1)


def _tiny():
    from qqq_amd import QuantLlamaForCausalLM

    cfg, gs = _config("llama", num_hidden_layers=1)
    return QuantLlamaForCausalLM.from_config(cfg, gs)


def test_generate_ragged_prompts_prefill_once_then_decode(monkeypatch):
    m = _tiny()
    stub = _Stub(m, monkeypatch)
    prompts = [[1, 2, 3], [10], [20, 21, 22, 23, 24, 25, 26]]
    out = m.generate(prompts, 4)
    assert out == [[4, 5, 6, 7], [11, 12, 13, 14], [27, 28, 29, 30]]
    assert [p["counts"] for p in stub.passes] == [[3, 1, 7], [1, 1, 1], [1, 1, 1], [1, 1, 1]]
    assert stub.passes[1]["starts"] == [3, 1, 7] and stub.passes[3]["starts"] == [5, 3, 9]
    assert m.generate(prompts, 0) == [[], [], []] and m.generate([], 3) == []
    with pytest.raises(ValueError, match="at least one token"):
        m.generate([[1], []], 2)


def test_generate_eos_in_the_middle_frees_the_blocks_at_once(monkeypatch):
    m = _tiny()
    stub = _Stub(m, monkeypatch)
    cache = m.new_cache(8, block_size=16)
    out = m.generate([[1, 2, 3], [10], [40]], 5, eos_token_id=12, cache=cache)
    assert out == [[4, 5, 6, 7, 8], [11, 12], [41, 42, 43, 44, 45]]  # the eos is part of the output
    assert [p["counts"] for p in stub.passes] == [[3, 1, 1], [1, 1, 1], [1, 1], [1, 1], [1, 1]]
    assert [p["free"] for p in stub.passes] == [5, 5, 6, 6, 6]  # sequence 1's block is back before the third pass
    assert cache.free_blocks == 8 and not cache._blocks
    # an eos as the very first token
    stub.passes.clear()
    assert m.generate([[11], [1]], 3, eos_token_id=12, cache=cache) == [[12], [2, 3, 4]]
    assert [p["counts"] for p in stub.passes] == [[1, 1], [1], [1]] and cache.free_blocks == 8


def test_generate_admits_the_rest_as_blocks_come_free(monkeypatch):
    m = _tiny()
    stub = _Stub(m, monkeypatch)
    prompts = [[1] * 20, [10] * 3, [30] * 17, [40]]  # budgets of 2, 1, 2 and 1 blocks of 16 (prompt + 5 new tokens - 1)
    roomy = m.generate(prompts, 5)
    stub.passes.clear()
    cache = m.new_cache(3, block_size=16)
    out = m.generate(prompts, 5, cache=cache)
    assert out == roomy == [[2, 3, 4, 5, 6], [11, 12, 13, 14, 15], [31, 32, 33, 34, 35], [41, 42, 43, 44, 45]]
    assert cache.free_blocks == 3 and not cache._blocks
    # the first two fit; the others wait, in order, until those finish; prefill and decode passes stay apart
    assert stub.passes[0]["counts"] == [20, 3]
    assert all(p["counts"] == [1, 1] for p in stub.passes[1:5])
    assert stub.passes[5]["counts"] == [17, 1] and stub.passes[5]["starts"] == [0, 0]
    assert all(p["free"] >= 0 for p in stub.passes)
    # other sequences in the caller's cache are left alone
    cache.add("mine")
    cache.step(["mine"], [16])
    assert m.generate(prompts[:2], 5, cache=cache) == roomy[:2] and cache.length("mine") == 16 and cache.free_blocks == 2
    with pytest.raises(RuntimeError, match="cannot hold a prompt"):
        m.generate([[1] * 40], 5, cache=cache)
    assert cache.free_blocks == 2
