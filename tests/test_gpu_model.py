"""QuantLlamaModel / QuantLlamaForCausalLM on the GPU: bit identity with the hand-built chain of layer.forward calls (the deferred residual),
generate() against a manual loop of forward + ops.sample_tokens, and the whole model against transformers' fp16 LlamaModel."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_attn import _fake_quant_linear, _make_layer

pytestmark = pytest.mark.gpu

HIDDEN, HEADS, KVH, INTER, VOCAB, LAYERS, D = 256, 4, 2, 512, 1000, 2, 64
PROMPT_LENS = (5, 17, 33)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _make_lm(dev, gs, seed=5):
    from qqq_amd import QuantLlamaForCausalLM, QuantLlamaModel

    layers = [_make_layer(dev, HIDDEN, HEADS, KVH, INTER, gs, False, seed + 10 * i) for i in range(LAYERS)]
    for i, layer in enumerate(layers):
        layer.self_attn.layer_idx = i
    lm = QuantLlamaForCausalLM(QuantLlamaModel(VOCAB, LAYERS, HIDDEN, HEADS, KVH, INTER, gs, rms_norm_eps=1e-6, layers=layers)).to(dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    lm.model.embed_tokens.weight.data = torch.randn((VOCAB, HIDDEN), generator=g, device=dev).half()
    lm.model.norm.weight.data = (1 + 0.1 * torch.randn(HIDDEN, generator=g, device=dev)).half()
    lm.lm_head.weight.data = (0.2 * torch.randn((VOCAB, HIDDEN), generator=g, device=dev)).half()
    return lm.eval()


def _prompts(seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in PROMPT_LENS]


def _chain(lm, ids, cache, step, rows=None):
    """embedding, layer.forward for each layer, the rows, ops.rmsnorm_quant's y, the head: the model without the deferred residual"""
    from qqq_amd import ops

    m = lm.model
    x = m.embed_tokens(ids)
    for layer in m.layers:
        x = layer(x, cache, step)
    x = x.reshape(-1, HIDDEN) if rows is None else x.reshape(-1, HIDDEN).index_select(0, rows)
    y = ops.rmsnorm_quant(x, m.norm.weight, m.norm.variance_epsilon, return_y=True)[2]
    return y, F.linear(y, lm.lm_head.weight)


@pytest.mark.parametrize("gs", [-1, 128])
@pytest.mark.parametrize("kind", ["static", "paged16", "paged8"])
def test_model_rows_are_bit_identical_to_the_chain_of_layer_forwards(dev, kind, gs):
    from qqq_amd import KVCache, PagedKVCache

    lm = _make_lm(dev, gs)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        if kind == "static":
            b = 2
            c_mod, c_ref = (KVCache(LAYERS, b, KVH, D, 32, dev) for _ in range(2))
            start = 0
            for s in (17, 1, 1):
                ids = torch.randint(0, VOCAB, (b, s), generator=g).to(dev)
                got = lm.model(ids, c_mod, start)
                last = torch.arange(b, device=dev) * s + (s - 1)
                want, want_logits = _chain(lm, ids, c_ref, start, last)
                assert got.shape == (b, HIDDEN) and torch.equal(_bits(got), _bits(want)), (s, start)
                for l in range(LAYERS):
                    assert torch.equal(_bits(c_mod.k[l]), _bits(c_ref.k[l])) and torch.equal(_bits(c_mod.v[l]), _bits(c_ref.v[l]))
                start += s
            ids = torch.randint(0, VOCAB, (b, 5), generator=g).to(dev)  # every row, and the logits
            got = lm(ids, c_mod, start, all_rows=True)
            assert got.shape == (b, 5, VOCAB) and torch.equal(_bits(got.reshape(-1, VOCAB)), _bits(_chain(lm, ids, c_ref, start)[1]))
            return
        dtype = torch.float16 if kind == "paged16" else torch.int8
        for fused in (False, True):
            lm.model.fuse_prefill() if fused else lm.model.unfuse_prefill()
            c_mod, c_ref = (PagedKVCache(LAYERS, 12, KVH, D, 16, dev, dtype=dtype) for _ in range(2))
            for c in (c_mod, c_ref):
                for sid in range(3):
                    c.add(sid)
            for counts in (PROMPT_LENS, (1, 1, 1), (1, 1, 1)):
                ids = torch.randint(0, VOCAB, (sum(counts),), generator=g).to(dev)
                s_mod, s_ref = c_mod.step([0, 1, 2], counts), c_ref.step([0, 1, 2], counts)
                got = lm(ids, c_mod, s_mod)
                rows = s_ref.cu_tokens[1:].long() - 1
                want, want_logits = _chain(lm, ids, c_ref, s_ref, rows)
                assert got.shape == (3, VOCAB) and torch.equal(_bits(got), _bits(want_logits)), (fused, counts)
                assert torch.isfinite(got).all()
            ids = torch.randint(0, VOCAB, (9,), generator=g).to(dev)  # a ragged chunk, every row
            counts = (2, 3, 4)
            got = lm.model(ids, c_mod, c_mod.step([0, 1, 2], counts), all_rows=True)
            assert got.shape == (9, HIDDEN) and torch.equal(_bits(got), _bits(_chain(lm, ids, c_ref, c_ref.step([0, 1, 2], counts))[0]))


def _manual(lm, prompts, n_new, T, k, p, seed, dtype=torch.float16):
    """prefill as one packed step, then decode steps: forward + ops.sample_tokens with generate()'s torch.rand draws"""
    from qqq_amd import ops

    dev = lm.lm_head.weight.device
    g = torch.Generator(device=dev).manual_seed(seed)
    cache = lm.new_cache(sum(-(-(len(q) + n_new - 1) // 16) for q in prompts), 16, dtype)
    sids = list(range(len(prompts)))
    for s in sids:
        cache.add(s)
    ids = torch.tensor([t for q in prompts for t in q], dtype=torch.int64, device=dev)
    counts = [len(q) for q in prompts]
    outs = []
    for _ in range(n_new):
        logits = lm(ids, cache, cache.step(sids, counts))
        u = torch.rand(len(sids), generator=g, device=dev)
        ids = ops.sample_tokens(logits, T, k, p, u)
        counts = [1] * len(sids)
        outs.append(ids.tolist())
    return [list(col) for col in zip(*outs)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_generate_equals_the_manual_loop_frees_its_blocks_and_survives_a_small_pool(dev, dtype):
    lm = _make_lm(dev, 128).fuse_prefill()
    prompts, n_new = _prompts(), 6
    with torch.no_grad():
        greedy = lm.generate(prompts, n_new, dtype=dtype)
        assert greedy == _manual(lm, prompts, n_new, 0.0, 0, 1.0, 0, dtype)
        assert all(len(o) == n_new and all(0 <= t < VOCAB for t in o) for o in greedy)
        for T, k, p in ((1.0, 0, 1.0), (0.8, 20, 0.9)):
            g = torch.Generator(device=dev).manual_seed(77)
            sampled = lm.generate(prompts, n_new, temperature=T, top_k=k, top_p=p, generator=g, dtype=dtype)
            assert sampled == _manual(lm, prompts, n_new, T, k, p, 77, dtype), (T, k, p)
        assert sampled != greedy  # 18 draws from distributions over 20 to 1000 tokens
        # an eos chosen from the first run: that sequence stops there, the others go on as before (rows are independent)
        eos = greedy[1][2]
        stopped = lm.generate(prompts, n_new, eos_token_id=eos, dtype=dtype)
        for got, full in zip(stopped, greedy):
            want = full[:full.index(eos) + 1] if eos in full else full
            assert got == want
        assert len(stopped[1]) <= 3
        # a caller's cache comes back with every block free; a pool too small for the three prompts gives the same tokens
        need = [-(-(len(q) + n_new - 1) // 16) for q in prompts]
        assert need == [1, 2, 3]
        roomy = lm.new_cache(sum(need), 16, dtype)
        assert lm.generate(prompts, n_new, cache=roomy) == greedy and roomy.free_blocks == sum(need)
        small = lm.new_cache(4, 16, dtype)
        assert lm.generate(prompts, n_new, cache=small) == greedy and small.free_blocks == 4
        assert lm.generate(prompts, n_new, eos_token_id=eos, cache=small) == stopped and small.free_blocks == 4


def test_model_against_transformers_fp16_llama(dev):
    """transformers' fp16 LlamaModel with the weights the QuantLinears hold (read back exactly: unit-row GEMMs) against the quantised model
    over a 33-token prompt.  The difference is the int8 per-token activation quantisation in front of every GEMM; the bound on the relative
    L2 error of the final normed hidden state is num_layers * 5e-2, the project's per-layer bound added linearly as the worst case.  A
    layout or naming error gives O(1).  Measured on an MI355X: 4.3e-4 and 4.7e-4 in two runs (the layers' norm weights are not seeded) (the residual stream is dominated by the unit-variance embedding
    rows, next to which these random layers' updates, and so their quantisation error, are small)."""
    tr = pytest.importorskip("transformers")
    from transformers.models.llama import modeling_llama as ml

    from qqq_amd import KVCache

    lm = _make_lm(dev, -1, seed=41)
    cfg = tr.LlamaConfig(vocab_size=VOCAB, hidden_size=HIDDEN, num_attention_heads=HEADS, num_key_value_heads=KVH, intermediate_size=INTER,
                         num_hidden_layers=LAYERS, rms_norm_eps=1e-6, max_position_embeddings=4096,
                         rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
    cfg._attn_implementation = "sdpa"
    ref = ml.LlamaModel(cfg).to(dev).half().eval()
    with torch.no_grad():
        ref.embed_tokens.weight.copy_(lm.model.embed_tokens.weight)
        ref.norm.weight.copy_(lm.model.norm.weight)
        for mine, theirs in zip(lm.model.layers, ref.layers):
            for name in ("q_proj", "k_proj", "v_proj", "o_proj"):
                getattr(theirs.self_attn, name).weight.copy_(_fake_quant_linear(getattr(mine.self_attn, name))[0])
            for name in ("gate_proj", "up_proj", "down_proj"):
                getattr(theirs.mlp, name).weight.copy_(_fake_quant_linear(getattr(mine.mlp, name))[0])
            theirs.input_layernorm.weight.copy_(mine.input_layernorm.weight)
            theirs.post_attention_layernorm.weight.copy_(mine.post_attention_layernorm.weight)
        ids = torch.tensor(_prompts()[2], dtype=torch.int64, device=dev)[None]
        want = ref(input_ids=ids, use_cache=False).last_hidden_state[0]
        got = lm.model(ids, KVCache(LAYERS, 1, KVH, D, 64, dev), 0, all_rows=True)[0]
    rel = float((got.float() - want.float()).norm() / want.float().norm())
    print(f"vs transformers LlamaModel ({LAYERS} layers, 33 tokens): relative L2 error of the final normed hidden state {rel:.2e}")
    assert torch.isfinite(got).all() and rel <= LAYERS * 5e-2, rel
