"""Sliding-window attention without a GPU: the per-layer windows from_config(..., sliding_window=True) derives from Mistral, Mixtral, Qwen2
and Qwen3 configs, the refusals of a windowed layer, and PagedKVCache.release_before's accounting."""
from types import SimpleNamespace

import pytest
import torch

BASE = dict(hidden_size=128, num_attention_heads=2, num_key_value_heads=2, intermediate_size=256, rms_norm_eps=1e-6, vocab_size=64,
            num_hidden_layers=2, hidden_act="silu", sliding_window=24)
CONFIGS = {
    "mistral": (dict(model_type="mistral"), [24, 24]),
    "mistral_null": (dict(model_type="mistral", sliding_window=None), [None, None]),
    "mixtral": (dict(model_type="mixtral", num_local_experts=2, num_experts_per_tok=1), [24, 24]),
    "qwen2": (dict(model_type="qwen2", use_sliding_window=True, max_window_layers=1), [None, 24]),
    "qwen2_off": (dict(model_type="qwen2", use_sliding_window=False, max_window_layers=0), [None, None]),
    "qwen3_types": (dict(model_type="qwen3", head_dim=64, layer_types=["sliding_attention", "full_attention"]), [24, None]),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_from_config_derives_the_window_of_every_layer(name):
    from qqq_amd import QuantLlamaForCausalLM

    over, want = CONFIGS[name]
    cfg = SimpleNamespace(**{**BASE, **over})
    lm = QuantLlamaForCausalLM.from_config(cfg, 128, sliding_window=True)
    assert [layer.self_attn.sliding_window for layer in lm.model.layers] == want
    assert lm.release_window() == (24 if all(w is not None for w in want) else None)
    if name == "mistral":  # without the keyword the window is ignored, as before
        plain = QuantLlamaForCausalLM.from_config(cfg, 128)
        assert [layer.self_attn.sliding_window for layer in plain.model.layers] == [None, None] and plain.release_window() is None


def test_a_windowed_layer_refuses_what_has_no_windowed_kernel():
    from qqq_amd import KVCache, QuantLlamaAttention, QuantLlamaDecoderLayer

    layer = QuantLlamaDecoderLayer(128, 2, 2, 256, 128, sliding_window=8)
    for what in ("fuse_verify", "fuse_shared"):
        with pytest.raises(NotImplementedError, match="sliding-window"):
            getattr(layer, what)()
    with pytest.raises(NotImplementedError, match="KVCache"):
        layer.self_attn.forward_int8(torch.zeros((1, 128), dtype=torch.int8), torch.ones((1, 1)), KVCache(1, 1, 2, 64, 16, "cpu"), 0)
    with pytest.raises(ValueError, match="at least 1"):
        QuantLlamaAttention(128, 2, 2, 128, sliding_window=0)


def test_release_before_gives_back_whole_blocks_and_respects_owners():
    from qqq_amd import PagedKVCache
    from qqq_amd.paged import RELEASED

    c = PagedKVCache(1, 8, 2, 64, 16, device="cpu")
    c.add("a")
    c.step(["a"], [40])                       # blocks 0, 1, 2
    c.fork("a", "b")                          # b shares 0 and 1, owns a copy of the partial block
    assert c.free_blocks == 4 and c.release_before("a", 31) == 1 and c.blocks("a") == [RELEASED, 1, 2]
    assert c.free_blocks == 4                 # block 0 has a second owner
    assert c.release_before("a", 33) == 1 and c.release_before("a", 33) == 0 and c.free_blocks == 4
    assert c.release_before("b", 16) == 1 and c.free_blocks == 5  # the last owner of block 0
    step = c.step(["a", "b"], [1, 9])         # lengths and positions are unchanged; released entries are written as 0
    assert step.starts == [40, 40] and c.length("a") == 41 and c.length("b") == 49
    assert step.block_table.tolist() == [[0, 0, 2, 0], [0, 1, c.blocks("b")[2], c.blocks("b")[3]]]
    assert step.slots[0].item() == 2 * 16 + 8
    with pytest.raises(ValueError, match="release_before"):
        c.gather(0, "a")
    assert c.release_before("a", 10 ** 6) == 1 and c.release_before("a", -5) == 0  # never beyond the blocks it holds
    c.free("a")
    c.free("b")
    assert c.free_blocks == 8 and sorted(c._free) == list(range(8)) and c._refs == [0] * 8
    with pytest.raises(KeyError):
        c.release_before("a", 1)
