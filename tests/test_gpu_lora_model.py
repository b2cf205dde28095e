"""Multi-LoRA through the layers and generate() on the GPU, on the two-layer model and the prompts of tests/test_gpu_model.py: a decoder
layer with step.lora against the hand composition of forward_int8 calls each followed by ops.lora_add (bit for bit, fused and unfused
holders, fp16 and int8 pools), and greedy generate() with mixed adapters against every prompt run alone, on the host path, DecodeLoop and
SpecDecodeLoop."""
import pytest
import torch

from test_gpu_model import HIDDEN, _make_lm, _prompts

pytestmark = pytest.mark.gpu

N_NEW, BS, ROWS, MAX_LEN, K = 10, 16, 3, 64, 2
PROJ = {"self_attn": ("q_proj", "k_proj", "v_proj", "o_proj"), "mlp": ("gate_proj", "up_proj", "down_proj")}
MIX = [0, None, 2, 0]


def _adapter(lm, seed, rank=8, b_zero=False, std=0.05, prefix="base_model.model.model.", only=None):
    """a PEFT-style state-dict of a random rank-`rank` adapter on all seven projections of every layer (B = 0: a freshly initialised one)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for li, layer in enumerate(lm.model.layers):
        for parent, names in PROJ.items():
            for name in (n for n in names if only is None or n in only):
                mod = getattr(getattr(layer, parent), name)
                key = f"{prefix}layers.{li}.{parent}.{name}"
                sd[key + ".lora_A.weight"] = torch.randn((rank, mod.infeatures), generator=g) * std
                sd[key + ".lora_B.weight"] = (torch.zeros((mod.outfeatures, rank)) if b_zero else
                                              torch.randn((mod.outfeatures, rank), generator=g) * std)
    return sd


def _bank(lm, slots=4, rank=16):
    from qqq_amd import LoraBank

    bank = LoraBank(lm, slots=slots, rank=rank)
    bank.load(0, _adapter(lm, 1), alpha=32)                      # rank 8 in a rank-16 bank: zero-padded
    bank.load(1, _adapter(lm, 2, b_zero=True), alpha=32)         # freshly initialised: B = 0
    bank.load(2, _adapter(lm, 3, rank=16, prefix=""), alpha=64)
    return bank


def _hand_layer(layer, x, cache, step, groups, slot):
    """QuantLlamaDecoderLayer.forward on a paged prefill step of a model with fuse_prefill(), from the single projections' forward_int8 each
    followed by ops.lora_add with the bank's per-projection views"""
    from qqq_amd import ops

    def lin(mod, name, xq, s1):
        y = mod.forward_int8(xq, s1)
        if name in groups:  # (a bank with fewer targets holds nothing for the others)
            A, B, scale, cols = groups[name]
            ops.lora_add(y, xq, s1.reshape(-1), A, B, scale, slot, cols)
        return y

    attn, mlp, li = layer.self_attn, layer.mlp, layer.self_attn.layer_idx
    x = x.reshape(-1, HIDDEN)
    xq, s1 = layer.input_layernorm(x)
    q, k, v = lin(attn.q_proj, "q_proj", xq, s1), lin(attn.k_proj, "k_proj", xq, s1), lin(attn.v_proj, "v_proj", xq, s1)
    cos, sin = attn.rope_tables(min(cache.capacity, max(1024, 1 << (step.max_len - 1).bit_length())))
    pools = (cache.k[li], cache.v[li]) + ((cache.k_scale[li], cache.v_scale[li]) if cache.quantized else ())
    q_out = (ops.rope_qkv_paged_kv8 if cache.quantized else ops.rope_qkv_paged)(q, k, v, cos, sin, step.pos, step.slots, *pools)
    prefill = ops.prefill_attention_paged_kv8 if cache.quantized else ops.prefill_attention_paged
    aq, a1 = prefill(q_out, *pools, step.block_table, step.cu_tokens, step.start_pos, attn.scaling, max_len=step.max_len)
    a = lin(attn.o_proj, "o_proj", aq, a1)
    mq, ms = layer.post_attention_layernorm(x, a)
    hq, hs = ops.silu_mul_quant(lin(mlp.gate_proj, "gate_proj", mq, ms), lin(mlp.up_proj, "up_proj", mq, ms))
    return a + lin(mlp.down_proj, "down_proj", hq, hs)


@pytest.mark.parametrize("pool", [torch.float16, torch.int8], ids=["fp16", "int8"])
@pytest.mark.parametrize("gs", [-1, 128])
def test_a_layer_with_step_lora_equals_the_hand_composition(dev, gs, pool, monkeypatch):
    from qqq_amd import ops

    lm = _make_lm(dev, gs).fuse_prefill()
    bank = _bank(lm)
    prompts = _prompts()
    counts = [len(p) for p in prompts]
    slots = [s for s, c in zip((0, -1, 2), counts) for _ in range(c)]
    slots[40] = 0  # a token of the last prompt on another adapter: the op is per token
    token_slot = bank.token_slots(slots)
    x = lm.model.embed_tokens(torch.tensor([t for p in prompts for t in p], device=dev))
    real, launched = ops.lora_add, []
    monkeypatch.setattr(ops, "lora_add", lambda *a, **k: (launched.append(1), real(*a, **k))[1])

    def fresh(lora):
        cache = lm.new_cache(8, BS, dtype=pool)
        for s in range(len(prompts)):
            cache.add(s)
        step = cache.step(list(range(len(prompts))), counts)
        step.lora = bank.step(token_slot) if lora else None
        return cache, step

    with torch.no_grad():
        for li, layer in enumerate(lm.model.layers):
            want = _hand_layer(layer, x.clone(), *fresh(True), bank.groups[li], token_slot)
            del launched[:]
            base = layer(x.clone(), *fresh(False))
            assert not launched and not torch.equal(base, want)  # without step.lora nothing of it runs; the adapters move the output
            got = layer(x.clone(), *fresh(True))
            assert len(launched) == 7 and torch.equal(got.view(torch.int16), want.view(torch.int16))
            layer.self_attn.fuse_qkv()
            layer.mlp.fuse_gate_up()
            del launched[:]
            fused = layer(x.clone(), *fresh(True))
            assert len(launched) == 4 and torch.equal(fused.view(torch.int16), want.view(torch.int16))
            layer.self_attn.unfuse_qkv()
            layer.mlp.unfuse_gate_up()


def test_a_fused_holder_with_part_of_its_group_targeted_adds_to_its_column_slices(dev, monkeypatch):
    """targets q, v and up only: the fused q|k|v and gate|up holders run the op on the targeted column slices of their outputs (row stride
    above N), bit for bit the hand composition and the unfused modules"""
    from qqq_amd import LoraBank, ops

    only = ("q_proj", "v_proj", "up_proj")
    lm = _make_lm(dev, 128).fuse_prefill()
    bank = LoraBank(lm, slots=3, rank=16, targets=only)
    bank.load(0, _adapter(lm, 1, only=only), alpha=32)
    bank.load(2, _adapter(lm, 3, rank=16, only=only), alpha=64)
    prompts = _prompts()
    counts = [len(p) for p in prompts]
    token_slot = bank.token_slots([s for s, c in zip((0, -1, 2), counts) for _ in range(c)])
    x = lm.model.embed_tokens(torch.tensor([t for p in prompts for t in p], device=dev))
    real, launched = ops.lora_add, []
    monkeypatch.setattr(ops, "lora_add", lambda *a, **k: (launched.append(a[0].stride(0) - a[0].shape[1]), real(*a, **k))[1])

    def fresh(lora=True):
        cache = lm.new_cache(8, BS)
        for s in range(len(prompts)):
            cache.add(s)
        step = cache.step(list(range(len(prompts))), counts)
        step.lora = bank.step(token_slot) if lora else None
        return cache, step

    with torch.no_grad():
        for li, layer in enumerate(lm.model.layers):
            assert set(bank.groups[li]) == set(only)
            want = _hand_layer(layer, x.clone(), *fresh(), bank.groups[li], token_slot)
            assert not torch.equal(want, layer(x.clone(), *fresh(False)))
            del launched[:]
            unfused = layer(x.clone(), *fresh())
            assert launched == [0, 0, 0] and torch.equal(unfused.view(torch.int16), want.view(torch.int16))
            layer.self_attn.fuse_qkv()
            layer.mlp.fuse_gate_up()
            del launched[:]
            fused = layer(x.clone(), *fresh())
            assert len(launched) == 3 and all(pad > 0 for pad in launched)  # three slices of wider outputs
            assert torch.equal(fused.view(torch.int16), want.view(torch.int16))


def _reference(lm, bank, prompts, adapters, n_new, pool=torch.float16):
    """generate()'s host path by hand, greedy: the prompts prefilled in one packed step, then one token per sequence and step, every step
    with the tokens' slots in step.lora -> (the tokens per prompt, {(prompt, position): the logits row the token there was drawn from})"""
    from qqq_amd import ops

    dev = lm.lm_head.weight.device
    slots = [-1 if a is None else a for a in adapters]
    cache = lm.new_cache(len(prompts) * (MAX_LEN // BS), BS, dtype=pool)
    for s in range(len(prompts)):
        cache.add(s)

    def step_of(counts):
        step = cache.step(list(range(len(prompts))), counts)
        step.lora = bank.step(bank.token_slots([slots[s] for s, c in enumerate(counts) for _ in range(c)]))
        return step

    logits = lm(torch.tensor([t for p in prompts for t in p], device=dev), cache, step_of([len(p) for p in prompts]))
    out, seen = [[] for _ in prompts], {}
    for j in range(n_new):
        toks = ops.sample_tokens(logits, 0.0, 0, 1.0, torch.zeros(len(prompts), device=dev))
        for s, t in enumerate(toks.tolist()):
            seen[(s, len(prompts[s]) + j)] = logits[s].float()
            out[s].append(t)
        if j + 1 < n_new:
            logits = lm(toks, cache, step_of([1] * len(prompts)))
    return out, seen


def _judge_of(lm, bank, prompts, adapters, n_new=N_NEW, pool=torch.float16):
    """-> (want, judge): the reference's greedy tokens, and the rule by which tests/test_gpu_spec_loop.py and test_gpu_penalty_loop.py compare
    a loop with it where the logits may differ in their last bits (a head GEMM or an attention kernel at another row count).  Strict
    equality would fail now and then: _make_layer draws the norm weights from the global generator, so an unseeded model, and with it the
    positions of its near-ties, differ from process to process (within a process every path here is bit for bit repeatable; _settled
    seeds the generator).  prompt +
    output are teacher-forced through one chunk with every row's logits and the same slots; D is the largest absolute difference between
    the logits the reference drew from and the teacher-forced ones.  judge(got): every emitted token's teacher-forced logit is within 2 D
    of its row's maximum, up to the first token that leaves the reference's (what follows is another sequence); the positions whose top-two
    margin is within 2 D -- where an argmax may legitimately differ -- are at most one in eight of all."""
    dev = lm.lm_head.weight.device
    want, seen = _reference(lm, bank, prompts, adapters, n_new, pool)
    slots = [-1 if a is None else a for a in adapters]
    full = [p + o for p, o in zip(prompts, want)]
    cache = lm.new_cache(len(prompts) * (MAX_LEN // BS), BS, dtype=pool)
    for s in range(len(full)):
        cache.add(s)
    step = cache.step(list(range(len(full))), [len(f) for f in full])
    step.lora = bank.step(bank.token_slots([slots[s] for s, f in enumerate(full) for _ in f]))
    forced = lm(torch.tensor([t for f in full for t in f], device=dev), cache, step, all_rows=True).float()
    offs = [0]
    for f in full:
        offs.append(offs[-1] + len(f))
    rows = {(s, q): forced[offs[s] + q - 1] for s in range(len(full)) for q in range(len(prompts[s]), len(full[s]))}  # row q - 1 predicts q
    d = max(float((seen[key] - rows[key]).abs().max()) for key in rows)
    margins = {key: float(torch.topk(row, 2).values.diff().abs()) for key, row in rows.items()}
    close = sum(m <= 2 * d for m in margins.values())
    print(f"adapters {adapters}: D {d:.4g}, smallest top-two margin {min(margins.values()):.4g} at {min(margins, key=margins.get)}, "
          f"{close} of {len(margins)} positions within 2 D")
    assert close * 8 <= len(margins), (close, d)

    def judge(got, what=""):
        flat = [o for g in got for o in (g if g and isinstance(g[0], list) else [g])]
        per = len(flat) // len(prompts)  # n completions per prompt
        for q, out in enumerate(flat):
            s = q // per
            assert len(out) == len(want[s]), (what, q, out)
            for j, t in enumerate(out):
                row = rows[(s, len(prompts[s]) + j)]
                assert float(row.max() - row[t]) <= 2 * d, (what, s, j, t, want[s][j], float(row.max() - row[t]), d)
                if t != want[s][j]:
                    print(f"{what}: prompt {s} token {j}: {t} for {want[s][j]}, margin {margins[(s, len(prompts[s]) + j)]:.4g}, D {d:.4g}")
                    break

    return want, judge


def _prompts4():
    p = _prompts()
    return p + [p[1][::-1][:9]]  # a fourth: one more than the small loops have rows


def _settled(dev, gs, pool=torch.float16):
    """(lm, bank, want, judge) for the adapters MIX on a model that is the same in every process: _make_lm under a seeded global generator
    (its norm weights come from it), the first seed whose reference run keeps the near-tie cap of _judge_of -- a property of the inputs,
    decided before any path under test runs"""
    for seed in range(8):
        with torch.random.fork_rng(devices=[dev]):
            torch.manual_seed(seed)
            lm = _make_lm(dev, gs).fuse_prefill()
        bank = _bank(lm)
        try:
            with torch.no_grad():
                return (lm, bank) + _judge_of(lm, bank, _prompts4(), MIX, pool=pool)
        except AssertionError as e:
            print("model seed", seed, "has too many near-ties:", e)
    raise AssertionError("no model seed whose near-tie positions are at most one in eight")


@pytest.fixture(scope="module")
def settled(dev):
    return _settled(dev, 128)


@pytest.fixture(scope="module")
def lm(settled):
    return settled[0]


@pytest.fixture(scope="module")
def bank(settled):
    return settled[1]


@pytest.fixture(scope="module")
def prompts():
    return _prompts4()


@pytest.fixture(scope="module")
def base(lm, prompts):
    with torch.no_grad():
        return lm.generate(prompts, N_NEW)


@pytest.fixture(scope="module")
def mix(settled):
    """(the greedy tokens with the adapters MIX, the rule a loop's tokens are held against): computed once, never changed"""
    return settled[2:]


@pytest.fixture(scope="module")
def mixed(mix):
    return mix[0]


def test_generate_is_the_reference_loop(lm, bank, prompts, mixed):
    """the host path runs the reference's steps at the reference's shapes: the same tokens"""
    with torch.no_grad():
        assert lm.generate(prompts, N_NEW, lora=bank, adapters=MIX) == mixed


def _alone_and_base(lm, bank, prompts, n_new, want, judge, **kw):
    """a mixed batch on the host path: the reference's tokens; every prompt run alone with its adapter: the same, by the rule of _judge_of
    (the fp16 head GEMM runs at one row there); None and a B = 0 adapter: the base model's tokens"""
    with torch.no_grad():
        base = lm.generate(prompts, n_new, **kw)
        mixed = lm.generate(prompts, n_new, lora=bank, adapters=MIX, **kw)
        print("base", base, "mixed", mixed)
        assert mixed == want
        judge([lm.generate([prompts[i]], n_new, lora=bank, adapters=[a], **kw)[0] for i, a in enumerate(MIX)], "every prompt alone")
        assert mixed[1] == base[1]                                                      # None: the base model
        assert mixed[0] != base[0] and mixed[2] != base[2]                              # a random adapter moves the logits
        assert lm.generate(prompts, n_new, lora=bank, adapters=[1] * 4, **kw) == base   # B = 0: the base model's tokens
        assert lm.generate(prompts, n_new, lora=bank, adapters=None, **kw) == base
        assert lm.generate(prompts, n_new, lora=bank, adapters=[2, 0, None, 2], **kw) != mixed


def test_a_mixed_batch_gives_every_prompt_the_tokens_it_gets_alone(lm, bank, prompts, mix):
    _alone_and_base(lm, bank, prompts, N_NEW, *mix)


def test_a_mixed_batch_per_channel_over_an_int8_pool(dev, prompts):
    """the same on per-channel weights and an int8 KV pool, and its device loop held against its own reference"""
    lm8, bank8, want, judge = _settled(dev, -1, pool=torch.int8)
    with torch.no_grad():
        _alone_and_base(lm8, bank8, prompts, N_NEW, want, judge, dtype=torch.int8)
        judge(lm8.generate(prompts, N_NEW, lora=bank8, adapters=MIX, dtype=torch.int8, device_loop=True), "device_loop, int8 pool")


def test_siblings_inherit_their_prompts_slot(lm, bank, prompts, mix):
    mixed, judge = mix
    with torch.no_grad():
        for kw in ({}, dict(device_loop=True)):  # eight rows: held against the four-row reference by the rule of _judge_of
            got = lm.generate(prompts, N_NEW, n=2, lora=bank, adapters=MIX, **kw)
            assert all(a == b for a, b in got) and got != lm.generate(prompts, N_NEW, n=2, **kw)  # greedy siblings: the same rows, on the adapter
            judge(got, f"n=2 {kw}")


def test_the_three_paths_agree(lm, bank, prompts, mix):
    """The host path is the reference (test_generate_is_the_reference_loop).  The loops are held against it by the rule of _judge_of: their
    head GEMM and attention run at other row counts (a chunk of K + 1 tokens per row, three rows for four prompts), so a logit may move by
    D and an argmax may differ where the top two are within 2 D; everywhere else the tokens are the reference's."""
    from qqq_amd import DecodeLoop, SpecDecodeLoop

    mixed, judge = mix
    with torch.no_grad():
        judge(lm.generate(prompts, N_NEW, lora=bank, adapters=MIX, device_loop=True), "device_loop")
        judge(lm.generate(prompts, N_NEW, lora=bank, adapters=MIX, device_loop=True, draft_len=K), "draft_len")
        for rows in (len(prompts), ROWS):  # the reference's row count, and one row fewer than prompts: a row is reused
            for graph in (False, True):
                loop = DecodeLoop(lm, lm.new_cache(rows * (MAX_LEN // BS), BS), rows=rows, max_len=MAX_LEN, sync_every=3, graph=graph, lora=bank)
                judge(loop.generate(prompts, N_NEW, adapters=MIX), f"DecodeLoop rows={rows} graph={graph}")
                assert bool((loop.lora_slot == -1).all())
                sloop = SpecDecodeLoop(lm, lm.new_cache(rows * (MAX_LEN // BS), BS), rows=rows, max_len=MAX_LEN, draft_len=K, sync_every=3,
                                       graph=graph, lora=bank)
                assert sloop.lora_slot.shape == (rows, K + 1)
                judge(sloop.generate(prompts, N_NEW, adapters=MIX), f"SpecDecodeLoop rows={rows} graph={graph}")
                assert bool((sloop.lora_slot == -1).all())


def test_a_load_between_two_calls_needs_no_new_capture(lm, prompts, mix, base):
    from qqq_amd import DecodeLoop

    own = _bank(lm)
    rows = len(prompts)
    with torch.no_grad():
        cache = lm.new_cache(rows * (MAX_LEN // BS), BS)
        nb = cache.free_blocks
        loop = DecodeLoop(lm, cache, rows=rows, max_len=MAX_LEN, sync_every=3, lora=own)
        addresses = [t.data_ptr() for t in own._storage]
        mix[1](loop.generate(prompts, N_NEW, adapters=MIX), "before the load")
        for seed in (7, 8, 9, 10):  # the first adapter whose reference run is no row of near-ties (the cap of _judge_of: a property of the inputs)
            own.load(3, _adapter(lm, seed, rank=4), alpha=16)
            try:
                want, judge = _judge_of(lm, own, prompts, [3] * 4)
                break
            except AssertionError as e:
                print("adapter seed", seed, "has too many near-ties:", e)
        else:
            raise AssertionError("no adapter whose near-tie positions are at most one in eight")
        assert want != mix[0] and want != base
        judge(loop.generate(prompts, N_NEW, adapters=[3] * 4), "after the load")
        own.unload(3)
        assert loop.generate(prompts, N_NEW, adapters=[3, None, 3, 3]) == base  # an emptied slot: the plain loop's tokens (test_gpu_stop_loop)
    assert loop.captures == 1 and cache.free_blocks == nb and addresses == [t.data_ptr() for t in own._storage]
    with pytest.raises(ValueError, match="adapters holds an entry that is neither None nor a slot in \\[0, 4\\)"):
        loop.generate(prompts, N_NEW, adapters=[4, 0, 0, 0])
    with pytest.raises(ValueError, match="adapters must hold one entry per prompt"):
        lm.generate(prompts, N_NEW, lora=own, adapters=[0])
    with pytest.raises(ValueError, match="adapters need lora"):
        lm.generate(prompts, N_NEW, adapters=MIX)


def test_without_lora_nothing_of_it_runs_or_is_allocated(lm, prompts, base, monkeypatch):
    from qqq_amd import DecodeLoop, ops

    def refuse(*a, **k):
        raise AssertionError("ops.lora_add ran without a bank")

    monkeypatch.setattr(ops, "lora_add", refuse)
    with torch.no_grad():
        assert lm.generate(prompts, N_NEW) == base and lm.generate(prompts, N_NEW, lora=None, adapters=None) == base
        loop = DecodeLoop(lm, lm.new_cache(ROWS * (MAX_LEN // BS), BS), rows=ROWS, max_len=MAX_LEN, sync_every=3)
        assert loop.generate(prompts, N_NEW) == base
    # no tensor of the feature exists: the loop has no lora_slot, its step and the cache's steps carry no LoraStep
    assert loop.lora is None and loop.step.lora is None and not hasattr(loop, "lora_slot")
    cache = lm.new_cache(2, BS)
    cache.add(0)
    assert cache.step([0], [3]).lora is None
    with pytest.raises(ValueError, match="adapters need a loop built with lora=bank"):
        loop.generate(prompts, N_NEW, adapters=MIX)
