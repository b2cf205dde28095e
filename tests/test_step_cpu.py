"""The decode loop's step without a GPU: PagedKVCache.reserve / advance, tests/step_ref.py against the allocator's own positions and
slots, the C-ABI of include/qqq_amd_step.h (declared set, exports, argument checks before any launch, the NULL no-op), the kernel's
resources in the gfx950 code object, and the op's CPU refusal and fake implementation."""
import os
import sys

import numpy as np
import pytest
import torch

import step_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 17
BS = 16


def _cache(num_blocks, **kw):
    from qqq_amd import PagedKVCache

    return PagedKVCache(1, num_blocks, 1, 64, BS, **kw)


# ---- reserve / advance

@pytest.mark.parametrize("start, new", [(5, 14), (15, 20), (16, 18), (1, 1), (16, 1), (33, 40)])
def test_reserved_stepping_equals_plain_stepping_on_a_fresh_pool(start, new):
    a, b = _cache(8), _cache(8)
    for c in (a, b):
        c.add("s")
    a.reserve("s", start + new)
    assert a.length("s") == 0 and len(a.blocks("s")) == -(-(start + new) // BS) and a.free_blocks == 8 - len(a.blocks("s"))
    owned = a.blocks("s")
    for count in [start] + [1] * new:
        sa, sb = a.step(["s"], [count]), b.step(["s"], [count])
        assert sa.pos.tolist() == sb.pos.tolist() and sa.slots.tolist() == sb.slots.tolist() and sa.starts == sb.starts
        assert sa.last_pos.tolist() == sb.last_pos.tolist() and sa.max_len == sb.max_len
        assert a.blocks("s") == owned  # nothing taken beyond the reservation
        assert sa.block_table[0, :len(b.blocks("s"))].tolist() == b.blocks("s")
    assert a.blocks("s") == b.blocks("s") and a.length("s") == b.length("s") == start + new
    a.step(["s"], [BS])  # beyond the reservation step() allocates as ever
    assert len(a.blocks("s")) == len(owned) + 1


def test_reserve_is_idempotent_and_never_shrinks():
    c = _cache(6)
    c.add(0)
    c.reserve(0, 40)
    blocks = c.blocks(0)
    assert len(blocks) == 3
    c.reserve(0, 40)
    c.reserve(0, 7)
    c.reserve(0, 0)
    assert c.blocks(0) == blocks and c.free_blocks == 3
    c.reserve(0, 49)
    assert c.blocks(0)[:3] == blocks and len(c.blocks(0)) == 4
    with pytest.raises(KeyError):
        c.reserve("nobody", 1)


def test_reserve_on_an_exhausted_pool_raises_and_changes_nothing():
    c = _cache(4)
    c.add(0)
    c.add(1)
    c.reserve(0, 3 * BS)
    free, mine = c.free_blocks, c.blocks(1)
    assert free == 1
    with pytest.raises(RuntimeError, match="exhausted"):
        c.reserve(1, BS + 1)
    assert c.free_blocks == free and c.blocks(1) == mine == [] and c.blocks(0) == [0, 1, 2]
    c.reserve(1, BS)  # what fits still fits
    assert c.free_blocks == 0


def test_free_returns_reserved_but_unused_blocks():
    c = _cache(5)
    c.add(0)
    c.reserve(0, 4 * BS)
    c.step([0], [3])  # one block in use, three reserved on top
    assert c.free_blocks == 1
    c.free(0)
    assert c.free_blocks == 5
    c.add(1)
    c.reserve(1, 5 * BS)
    assert sorted(c.blocks(1)) == [0, 1, 2, 3, 4]


def test_advance_moves_the_length_inside_the_reservation_only():
    c = _cache(4)
    c.add(0)
    c.reserve(0, 40)  # three blocks: 48 keys
    c.step([0], [5])
    c.advance(0, 30)
    assert c.length(0) == 35
    k, v = c.gather(0, 0)
    assert k.shape == (1, 1, 35, 64) and v.shape == (1, 1, 35, 64)
    with pytest.raises(ValueError, match="advance"):
        c.advance(0, 14)  # 49 keys: past the three blocks
    with pytest.raises(ValueError, match="advance"):
        c.advance(0, -1)
    assert c.length(0) == 35
    c.advance(0, 13)
    assert c.length(0) == 48
    st = c.step([0], [1])  # a later step goes on where the device stopped, into a new block
    assert st.pos.tolist() == [48] and st.slots.tolist() == [c.blocks(0)[3] * BS] and len(c.blocks(0)) == 4
    with pytest.raises(KeyError):
        c.advance("nobody", 1)


# ---- the reference against the allocator

STARTS, BUDGETS = (5, 15, 16), (14, 20, 18)  # budgets that cross one block boundary (5 -> 18), two (15 -> 34) and one at once (16 -> 33)


def _reserved_state(table_stride=3, out_stride=32):
    c = _cache(9)
    for s in range(3):
        c.add(s)
    c.step([0, 1, 2], STARTS)  # the prompts
    for s in (2, 0, 1):  # in an order of its own, so that the tables interleave
        c.reserve(s, STARTS[s] + BUDGETS[s])
    st = step_ref.new_state(3, table_stride, out_stride, BS)
    for s in range(3):
        blocks = c.blocks(s)
        st["block_table"][s, :len(blocks)] = blocks
        st["pos"][s] = STARTS[s]
        st["slots"][s] = blocks[STARTS[s] // BS] * BS + STARTS[s] % BS
        st["remaining"][s] = BUDGETS[s]
        st["ids"][s] = 100 + s
    return c, st


def test_reference_trajectory_equals_the_allocators_steps():
    c, st = _reserved_state()
    assert [len(c.blocks(s)) for s in range(3)] == [2, 3, 3]
    rng = np.random.default_rng(3)
    emitted = [[] for _ in range(3)]
    for j in range(max(BUDGETS) + 2):
        live = [s for s in range(3) if j < BUDGETS[s]]
        assert [s for s in range(3) if st["remaining"][s] > 0] == live
        if live:
            want = c.step(live, [1] * len(live))  # the reserved blocks serve: nothing new is taken
            assert st["pos"][live].tolist() == want.pos.tolist() == want.last_pos.tolist()
            assert st["slots"][live].tolist() == want.slots.tolist()
        idle = [s for s in range(3) if s not in live]
        assert (st["pos"][idle] == -1).all() and (st["slots"][idle] == -1).all() and (st["ids"][idle] == 0).all()
        toks = rng.integers(0, 1000, 3)
        before = step_ref.copy_state(st)
        step_ref.advance(st, toks)
        for s in live:
            emitted[s].append(int(toks[s]))
            if j + 1 < BUDGETS[s]:
                assert st["ids"][s] == toks[s] and st["remaining"][s] == BUDGETS[s] - j - 1
        for s in idle:
            for f in ("ids", "pos", "slots", "remaining", "n_out", "out"):
                assert np.array_equal(st[f][s], before[f][s]), f
        assert (st["tick"] == j + 1).all()
    assert c.free_blocks == 9 - 8
    for s in range(3):
        assert st["n_out"][s] == BUDGETS[s] and st["out"][s, :BUDGETS[s]].tolist() == emitted[s]
        assert c.length(s) == STARTS[s] + BUDGETS[s]


def test_reference_eos_at_the_second_token_retires_the_row_for_good():
    _, st = _reserved_state()
    st["eos"][1] = 777
    step_ref.advance(st, [1, 2, 3])
    assert st["remaining"].tolist() == [13, 19, 17] and st["pos"].tolist() == [6, 16, 17]
    step_ref.advance(st, [4, 777, 777])  # row 2 has no eos: 777 is a token like any other
    assert st["remaining"].tolist() == [12, 0, 16]
    assert (st["pos"][1], st["slots"][1], st["ids"][1], st["n_out"][1]) == (-1, -1, 0, 2) and st["out"][1, :2].tolist() == [2, 777]
    assert st["ids"][2] == 777 and st["pos"][2] == 18
    frozen = st["out"][1].copy()
    for j in range(3):
        step_ref.advance(st, [9, 777, 9])
        assert np.array_equal(st["out"][1], frozen) and st["n_out"][1] == 2 and st["pos"][1] == -1 and st["remaining"][1] == 0
    assert st["tick"].tolist() == [5, 5, 5]


def test_reference_retires_instead_of_leaving_out_or_the_table():
    # out_stride 4 with a budget of 14: the fourth token fills out and retires the row
    _, st = _reserved_state(out_stride=4)
    for j in range(6):
        step_ref.advance(st, [10 + j] * 3)
    assert st["n_out"].tolist() == [4, 4, 4] and (st["remaining"] == 0).all() and (st["pos"] == -1).all()
    assert st["out"].tolist() == [[10, 11, 12, 13]] * 3
    # a table of 2 blocks under budgets that need 3: rows 1 and 2 retire with the token whose successor would sit at position 32
    c, st = _reserved_state(table_stride=3)
    st["block_table"] = np.ascontiguousarray(st["block_table"][:, :2])
    st["remaining"][:] = 10 ** 6  # a corrupt budget
    for j in range(40):
        step_ref.advance(st, [5] * 3)
        live = st["remaining"] > 0
        assert (st["pos"][live] < 32).all() and (st["pos"][live] >= 0).all()
        for s in np.nonzero(live)[0]:
            assert st["slots"][s] == c.blocks(s)[st["pos"][s] // BS] * BS + st["pos"][s] % BS
    assert (st["remaining"] == 0).all() and st["n_out"].tolist() == [32 - 5, 32 - 15, 32 - 16]
    # state no caller reaches: a count outside out writes nothing and retires
    _, st = _reserved_state(out_stride=4)
    st["n_out"][0], st["n_out"][1] = 4, -1
    before = st["out"].copy()
    step_ref.advance(st, [1, 2, 3])
    assert np.array_equal(st["out"][:2], before[:2]) and st["remaining"].tolist()[:2] == [0, 0] and st["n_out"].tolist() == [4, -1, 1]


# ---- the C-ABI

@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def test_header_declares_the_entry_and_the_library_exports_it(L):
    from qqq_amd import _abi

    names = set(_abi.prototypes(os.path.join(ROOT, "include", "qqq_amd_step.h")))
    assert names == {"qqq_sample_advance"}
    for n in names:
        assert hasattr(L, n), n
    assert L.qqq_amd_abi_version() == 4
    main = _abi.source(os.path.join(ROOT, "include", "qqq_amd.h"))
    assert "qqq_sample_advance" not in main and "qqq_step" not in main  # the feature has its own header


# fake device addresses with the alignment the entry point asks for: the calls below must fail in the checks, before any launch
A16, A8, A4 = 0x10000, 0x20008, 0x30004
PTRS = dict(logits=A16, T=A4, k=A4, p=A4, u=A4, tick=A4, ids=A8, pos=A8, slots=A8, table=A4, remaining=A4, eos=A4, out=A8, n_out=A4)


def _call(L, ld=1008, u_stride=3, table_stride=3, out_stride=4, rows=6, vocab=1003, block_size=16, **ptrs):
    a = dict(PTRS, **ptrs)
    return L.qqq_sample_advance(a["logits"], ld, a["T"], a["k"], a["p"], a["u"], u_stride, a["tick"], a["ids"], a["pos"], a["slots"],
                                a["table"], table_stride, a["remaining"], a["eos"], a["out"], out_stride, a["n_out"], rows, vocab,
                                block_size, 0, None)


BAD = ([{name: None} for name in PTRS] + [dict(logits=A16 + 8)] + [{name: A8 + 4} for name in ("ids", "pos", "slots", "out")]
       + [{name: A4 + 2} for name in ("T", "k", "p", "u", "tick", "table", "remaining", "eos", "n_out")]
       + [dict(block_size=b) for b in (24, 8, 512, 0, -16)] + [dict(u_stride=0), dict(table_stride=0), dict(out_stride=0),
                                                                dict(u_stride=-1), dict(table_stride=-3), dict(out_stride=-1)]
       + [dict(ld=1003), dict(ld=1000), dict(vocab=0, ld=8), dict(vocab=262145, ld=262152), dict(rows=-1), dict(rows=65536)])


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_sample_advance_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _call(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_sample_advance:")


def test_rows_0_is_a_no_op_with_null_pointers(L):
    z = None
    assert L.qqq_sample_advance(z, 0, z, z, z, z, 0, z, z, z, z, z, 0, z, z, z, 0, z, 0, 1003, 16, 0, z) == 0
    assert L.qqq_sample_advance(z, 0, z, z, z, z, 0, z, z, z, z, z, 0, z, z, z, 0, z, 0, 0, 0, 0, z) == 0
    assert _call(L, rows=0) == 0


def test_step_kernel_in_the_code_object_without_scratch_or_spills():
    """The sampler's kernel is what it was (tests/test_sample_cpu.py pins its name and budget); the step kernel shares its body and stays
    inside the same budget: sixteen waves, no scratch, registers and LDS for two workgroups per CU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB)}
    step = ks["qqq_step_advance_kernel"]
    assert step["private_segment_fixed_size"] == 0 and step["vgpr_spill_count"] == 0 and step["sgpr_spill_count"] == 0, step
    assert step["max_flat_workgroup_size"] == 1024 and step["vgpr_count"] + step["agpr_count"] <= 128, step
    assert step["group_segment_fixed_size"] == ks["qqq_sample_tokens_kernel"]["group_segment_fixed_size"] <= 80 * 1024


# ---- the op without a GPU

def _op_args(rows=3, vocab=40, u_stride=2, width=2, out_stride=5):
    i32, i64 = torch.int32, torch.int64
    return dict(logits=torch.zeros((rows, vocab), dtype=torch.float16), temperature=1.0, top_k=0, top_p=1.0, u=torch.zeros((rows, u_stride)),
                tick=torch.zeros(rows, dtype=i32), ids=torch.zeros(rows, dtype=i64), pos=torch.zeros(rows, dtype=i64),
                slots=torch.zeros(rows, dtype=i64), block_table=torch.zeros((rows, width), dtype=i32), remaining=torch.zeros(rows, dtype=i32),
                eos=torch.zeros(rows, dtype=i32), out=torch.zeros((rows, out_stride), dtype=i64), n_out=torch.zeros(rows, dtype=i32),
                block_size=16)


def test_cpu_tensors_raise_and_shapes_are_checked():
    import qqq_amd
    from qqq_amd import ops

    assert qqq_amd.sample_advance is ops.sample_advance and qqq_amd.DecodeLoop is not None
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sample_advance(**_op_args())
    with pytest.raises(RuntimeError, match="temperature holds 2 entries"):
        ops.sample_advance(**dict(_op_args(), temperature=torch.ones(2)))
    with pytest.raises(RuntimeError, match=r"fp16 \[rows, vocab\]"):
        ops.sample_advance(**dict(_op_args(), logits=torch.zeros(40, dtype=torch.float16)))


def test_fake_implementation_checks_dtypes_and_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from qqq_amd import ops

    with FakeTensorMode():
        assert ops.sample_advance(**_op_args()) is None
        for bad, msg in ((dict(pos=torch.zeros(3, dtype=torch.int32)), "pos must be int64"), (dict(tick=torch.zeros(4, dtype=torch.int32)), "tick"),
                         (dict(u=torch.zeros(3)), "u must be f32"), (dict(out=torch.zeros(3, dtype=torch.int64)), "out must be int64"),
                         (dict(block_table=torch.zeros((2, 2), dtype=torch.int32)), "block_table"), (dict(block_size=24), "block_size")):
            with pytest.raises(RuntimeError, match=msg):
                ops.sample_advance(**dict(_op_args(), **bad))


# ---- DecodeLoop: the host's bookkeeping, with host stubs for the forward pass and the two sampler ops

class _LoopStub:
    """forward: logits whose argmax is (the row's input token + 1) % 50; sample_tokens: argmax; sample_advance: argmax + step_ref.advance on
    the loop's own (CPU) arrays.  Checks every decode pass's positions and slots against the sequences' reserved blocks."""

    def __init__(self, m, monkeypatch):
        self.m, self.decode_passes, self.prefills, self.cache, self.free_seen, self.variates = m, 0, [], None, [], []
        monkeypatch.setattr(m, "forward", self.forward)
        monkeypatch.setattr("qqq_amd.serve.ops.sample_tokens", lambda logits, T, k, p, u: logits.argmax(dim=1))
        monkeypatch.setattr("qqq_amd.serve.ops.sample_advance", self.advance)

    def forward(self, ids, cache, step, all_rows=False):
        assert ids.dtype == torch.int64 and ids.shape == (sum(step.counts),)
        self.free_seen.append(cache.free_blocks)
        if step.pos is step.last_pos:  # the loop's own step
            assert step.decode and step.counts == [1] * ids.shape[0] and step.slots.shape == ids.shape
            self.decode_passes += 1
            bs = cache.block_size
            for r, (p, s) in enumerate(zip(step.pos.tolist(), step.slots.tolist())):
                assert (p, s) == (-1, -1) or s == int(step.block_table[r, p // bs]) * bs + p % bs
                assert p < step.max_len
            return torch.nn.functional.one_hot((ids + 1) % 50, 50).half()
        self.prefills.append(list(step.counts))
        return torch.nn.functional.one_hot((ids[step.cu_tokens[1:].long() - 1] + 1) % 50, 50).half()

    def advance(self, logits, T, k, p, u, tick, ids, pos, slots, block_table, remaining, eos, out, n_out, block_size):
        assert u.shape[0] == logits.shape[0] and int(tick.max()) < u.shape[1]  # a variate is never used twice
        self.variates.append(u.gather(1, tick.long()[:, None])[:, 0].tolist())
        st = dict(tick=tick.numpy(), ids=ids.numpy(), pos=pos.numpy(), slots=slots.numpy(), block_table=block_table.numpy(),
                  remaining=remaining.numpy(), eos=eos.numpy(), out=out.numpy(), n_out=n_out.numpy(), block_size=block_size)
        step_ref.advance(st, logits.argmax(dim=1).tolist())


def _tiny_lm():
    from types import SimpleNamespace

    from qqq_amd import QuantLlamaForCausalLM

    cfg = SimpleNamespace(vocab_size=50, hidden_size=128, num_attention_heads=2, num_key_value_heads=2, intermediate_size=256,
                          num_hidden_layers=1, rms_norm_eps=1e-6, hidden_act="silu", rope_theta=10000.0, max_position_embeddings=512,
                          attention_bias=False, mlp_bias=False, tie_word_embeddings=False, pad_token_id=None, model_type="llama")
    return QuantLlamaForCausalLM.from_config(cfg, -1)


def _run_up(first, n):
    return [(first + j) % 50 for j in range(n)]


def test_decode_loop_bookkeeping_with_host_stubs(monkeypatch):
    from qqq_amd import DecodeLoop

    m = _tiny_lm()
    stub = _LoopStub(m, monkeypatch)
    cache = m.new_cache(6, 16)
    loop = DecodeLoop(m, cache, rows=2, max_len=48, sync_every=3, u_stride=4, graph=False)
    assert loop.step.pos is loop.step.last_pos is loop.step.start_pos is loop.pos and loop.block_table.shape == (2, 3)
    prompts = [[1, 2, 3], [10] * 17, [20] * 30, [7], [30, 31]]
    # budgets of 1, 2, 3, 1 and 1 blocks through two rows and six blocks: the third prompt waits for a row
    out = loop.generate(prompts, 9)
    assert out == [_run_up(4, 9), _run_up(11, 9), _run_up(21, 9), _run_up(8, 9), _run_up(32, 9)]
    assert cache.free_blocks == 6 and stub.prefills[0] == [3, 17] and sorted(c for p in stub.prefills for c in p) == [1, 2, 3, 17, 30]
    assert (loop.remaining == 0).all() and (loop.pos == -1).all() and (loop.slots == -1).all() and loop.captures == 0
    assert min(stub.free_seen) >= 0
    # an eos ends a sequence with the eos in its output; a budget of 1 never decodes; the rows are reused by the next call
    passes = stub.decode_passes
    assert loop.generate(prompts[:2], 9, eos_token_id=6) == [[4, 5, 6], _run_up(11, 9)] and cache.free_blocks == 6
    assert loop.generate(prompts[:2], 9, eos_token_id=4) == [[4], _run_up(11, 9)]
    before = stub.decode_passes
    assert loop.generate(prompts, 1) == [[4], [11], [21], [8], [32]] and stub.decode_passes == before and before > passes
    assert loop.generate(prompts, 0) == [[]] * 5 and loop.generate([], 3) == []
    # the decode passes of one sequence: 8 tokens in rounds of sync_every = 3, the last one cut to what is left
    before = stub.decode_passes
    assert loop.generate([[5]], 9) == [_run_up(6, 9)] and stub.decode_passes - before == 8


def test_decode_loop_draws_depend_on_the_calls_generator_alone(monkeypatch):
    """Two loops with different histories (one served a greedy call first, whose variates came from the default generator) see the same
    variates in a call with equally seeded generators; no variate of the earlier call is left over."""
    from qqq_amd import DecodeLoop

    m = _tiny_lm()
    stub = _LoopStub(m, monkeypatch)
    seen = []
    for warm in (False, True):
        loop = DecodeLoop(m, m.new_cache(4, 16), rows=2, max_len=32, sync_every=3, u_stride=4, graph=False)
        if warm:
            loop.generate([[1, 2]], 6)
        stub.variates.clear()
        loop.generate([[1, 2], [3]], 9, temperature=1.0, generator=torch.Generator().manual_seed(5))
        seen.append(list(stub.variates))
    assert seen[0] == seen[1] and len(seen[0]) == 8 and len({v for step in seen[0] for v in step}) == 16


def test_decode_loop_refusals_leave_the_pool_alone(monkeypatch):
    from qqq_amd import DecodeLoop

    m = _tiny_lm()
    _LoopStub(m, monkeypatch)
    cache = m.new_cache(4, 16)
    loop = DecodeLoop(m, cache, rows=2, max_len=48, graph=False)
    with pytest.raises(ValueError, match="max_len=48"):
        loop.generate([[1], [2] * 40], 10)  # 49 keys
    with pytest.raises(ValueError, match="at least one token"):
        loop.generate([[1], []], 3)
    cache.add("other")
    cache.reserve("other", 33)  # three of the four blocks
    with pytest.raises(RuntimeError, match="cannot hold a prompt"):
        loop.generate([[1] * 3, [2] * 20], 4)  # the first runs and finishes, the second needs two blocks
    assert cache.free_blocks == 1 and (loop.remaining == 0).all() and (loop.pos == -1).all()
    with pytest.raises(ValueError, match="u_stride"):
        DecodeLoop(m, cache, rows=2, max_len=48, sync_every=8, u_stride=7, graph=False)
    with pytest.raises(ValueError, match="exceeds what the pool could hold"):
        DecodeLoop(m, cache, rows=2, max_len=65, graph=False)
    with pytest.raises(RuntimeError, match="graph=True needs the model on the GPU"):
        DecodeLoop(m, cache, rows=2, max_len=48)
    with pytest.raises(TypeError):
        DecodeLoop(m, object(), rows=2, max_len=48, graph=False)


def test_generate_device_loop_delegates_to_a_decode_loop(monkeypatch):
    m = _tiny_lm()
    made = []

    class _Loop:
        def __init__(self, lm, cache, rows, max_len):
            made.append((lm, cache.num_blocks, rows, max_len))

        def generate(self, *a):
            return ["delegated", a]

    monkeypatch.setattr("qqq_amd.serve.DecodeLoop", _Loop)
    prompts = [[1, 2, 3], [4] * 20]
    got = m.generate(prompts, 9, 0.5, 7, 0.9, None, 3, device_loop=True)
    assert got == ["delegated", (prompts, 9, 0.5, 7, 0.9, None, 3)]
    assert made == [(m, 1 + 2, 2, 32)]  # budgets of 11 and 28 keys: 1 + 2 blocks, the longest rounded up to a block
    m.generate([[1]] * 70, 2, device_loop=True)
    assert made[1][2] == 64
