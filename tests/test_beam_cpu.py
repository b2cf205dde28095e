"""Beam search without a GPU: what the header declares and how it is bound, the C-ABI's argument checks before any launch, the kernels'
resources in the gfx950 code object, the ops' CPU refusal and fake implementations, tests/beam_ref.py on hand-made cases,
PagedKVCache.reorder on CPU pools, and QuantLlamaForCausalLM.beam_search over a stub model with ops.beam_step replaced by the reference."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import beam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qqq_amd_beam.h")
ERR_ARG = 17


@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


# ---- the header and its binding

def test_the_header_declares_the_three_entries(L):
    from qqq_amd import _abi, _lib, build

    assert _lib.ABI_VERSION == 4 and L.qqq_amd_abi_version() == 4
    protos = _abi.prototypes(HEADER)
    assert set(protos) == {"qqq_beam_step", "qqq_beam_step_workspace_bytes", "qqq_copy_blocks"}
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[ret] and len(fn.argtypes) == len(params), name
        assert all(p.rsplit(" ", 1)[0] in ("const void*", "void*", "int", "size_t") for p in params), params
    unit = open(build.SRC).read()
    assert '#include "qqq_beam.hip.h"' in unit and '#include "../../include/qqq_amd_beam.h"' in unit
    assert unit.index('#include "qqq_logprobs.hip.h"') < unit.index('#include "qqq_beam.hip.h"')
    kernels = open(os.path.join(os.path.dirname(build.SRC), "qqq_beam.hip.h")).read()
    assert "qqq_logprobs_row(" in kernels and "qqq_sample_select" not in kernels  # the row body is called, not copied
    main = _abi.source(build.header("qqq_amd.h"))
    assert "qqq_beam" not in main and "qqq_copy_blocks" not in main


# ---- the C ABI: fake device addresses with the alignment the entries ask for; every call below must fail in the checks, before any launch
A16, A8, A4 = 0x10000, 0x20008, 0x30004
STEP = dict(logits=A16, cum=A4, live=A4, cand_score=A4, cand_logprob=A4, cand_parent=A4, cand_token=A4, next_ids=A8, next_parent=A4,
            next_cum=A4, next_live=A4, workspace=A4)
COPY = dict(pools=A8, src=A4, dst=A4)


def _step(L, ld=1008, ws_bytes=None, B=4, eos=2, rows=12, vocab=1003, **ptrs):
    a = dict(STEP, **ptrs)
    if ws_bytes is None:
        ws_bytes = max(L.qqq_beam_step_workspace_bytes(rows, B), 16)
    return L.qqq_beam_step(a["logits"], ld, a["cum"], a["live"], a["cand_score"], a["cand_logprob"], a["cand_parent"], a["cand_token"],
                           a["next_ids"], a["next_parent"], a["next_cum"], a["next_live"], a["workspace"], ws_bytes, B, eos, rows, vocab, 0, None)


def _copy(L, n_pools=4, n=3, block_bytes=4096, num_blocks=8, **ptrs):
    a = dict(COPY, **ptrs)
    return L.qqq_copy_blocks(a["pools"], n_pools, a["src"], a["dst"], n, block_bytes, num_blocks, 0, None)


BAD_STEP = ([{name: None} for name in STEP] + [dict(logits=A16 + 8), dict(next_ids=A8 + 4)]
            + [{name: A4 + 2} for name in STEP if STEP[name] == A4]
            + [dict(B=0, rows=0), dict(B=17, rows=17), dict(B=-1), dict(B=16, rows=16, vocab=31, ld=32), dict(B=4, vocab=7, ld=8),
               dict(ld=1002), dict(ld=1000), dict(ld=1004), dict(ld=1012), dict(ld=-1008), dict(vocab=262145, ld=262152), dict(rows=-4), dict(rows=65536),
               dict(rows=65536, B=16), dict(rows=13), dict(ws_bytes=12 * 8 * 8 - 4), dict(ws_bytes=0)])
BAD_COPY = ([{name: None} for name in COPY] + [dict(pools=A8 + 4), dict(src=A4 + 2), dict(dst=A4 + 2)]
            + [dict(block_bytes=b) for b in (0, 8, 24, 4100)] + [dict(n=-1), dict(n_pools=0), dict(n_pools=65536), dict(num_blocks=0)])


@pytest.mark.parametrize("kw", BAD_STEP, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_beam_step_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _step(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_beam_step:"), _lib.last_error()


@pytest.mark.parametrize("kw", BAD_COPY, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_copy_blocks_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _copy(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_copy_blocks:"), _lib.last_error()


def test_rows_0_and_n_0_are_no_ops_with_null_pointers(L):
    z = None
    assert L.qqq_beam_step(z, 0, z, z, z, z, z, z, z, z, z, z, z, 0, 4, -1, 0, 0, 0, z) == 0
    assert _step(L, rows=0) == 0
    assert L.qqq_copy_blocks(z, 0, z, z, 0, 0, 0, 0, z) == 0 and _copy(L, n=0) == 0
    assert L.qqq_beam_step_workspace_bytes(12, 4) == 12 * 8 * 8 and L.qqq_beam_step_workspace_bytes(65535, 15) == 65535 * 30 * 8
    for rows, B in ((0, 4), (13, 4), (17, 17), (4, 0), (65536, 16)):
        assert L.qqq_beam_step_workspace_bytes(rows, B) == 0


def test_beam_kernels_in_the_code_object_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB)}
    for name, threads in (("qqq_beam_rows_kernel", 1024), ("qqq_beam_merge_kernel", 256), ("qqq_copy_blocks_kernel", 256)):
        k = ks[name]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["max_flat_workgroup_size"] == threads, k
    # the rows kernel is the top-k kernel's row body and nothing else
    assert ks["qqq_beam_rows_kernel"]["group_segment_fixed_size"] == ks["qqq_topk_kernel"]["group_segment_fixed_size"]
    assert ks["qqq_beam_rows_kernel"]["vgpr_count"] <= 128 and ks["qqq_beam_merge_kernel"]["vgpr_count"] <= 64


# ---- the ops layer

def _step_args(rows=8, B=4, vocab=40):
    return dict(logits=torch.zeros((rows, vocab), dtype=torch.float16), cum=torch.zeros(rows), live=torch.ones(rows, dtype=torch.int32),
                num_beams=B, eos=3)


def _copy_args(n=3):
    return dict(pools=torch.zeros(4, dtype=torch.int64), src=torch.zeros(n, dtype=torch.int32), dst=torch.ones(n, dtype=torch.int32),
                block_bytes=4096, num_blocks=8)


def test_ops_are_exported_and_have_no_cpu_path():
    import qqq_amd
    from qqq_amd import ops

    assert qqq_amd.beam_step is ops.beam_step and qqq_amd.copy_blocks is ops.copy_blocks
    assert qqq_amd.BeamHypothesis is qqq_amd.beam.BeamHypothesis
    assert {"beam_step", "copy_blocks", "BeamHypothesis"} <= set(qqq_amd.__all__)
    with pytest.raises(RuntimeError, match="beam_step: .*no CPU path"):
        ops.beam_step(**_step_args())
    with pytest.raises(RuntimeError, match="copy_blocks: .*no CPU path"):
        ops.copy_blocks(**_copy_args())
    with pytest.raises(RuntimeError, match="beam_step: logits must be"):
        ops.beam_step(**dict(_step_args(), logits=torch.zeros(40, dtype=torch.float16)))


def test_fake_implementations_check_dtypes_and_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from qqq_amd import ops

    with FakeTensorMode():
        out = ops.beam_step(**_step_args())
        assert isinstance(out, ops.BeamStep)
        for name, shape, dt in (("cand_score", (2, 8), torch.float32), ("cand_logprob", (2, 8), torch.float32),
                                ("cand_parent", (2, 8), torch.int32), ("cand_token", (2, 8), torch.int32), ("next_ids", (8,), torch.int64),
                                ("next_parent", (8,), torch.int32), ("next_cum", (8,), torch.float32), ("next_live", (8,), torch.int32),
                                ("packed", (72,), torch.int32)):
            t = getattr(out, name)
            assert tuple(t.shape) == shape and t.dtype == dt, name
        for bad, err, msg in ((dict(cum=torch.zeros(8, dtype=torch.float64)), RuntimeError, "cum must be f32"),
                              (dict(cum=torch.zeros(7)), RuntimeError, "cum must be f32"),
                              (dict(live=torch.ones(8, dtype=torch.int64)), RuntimeError, "live must be int32"),
                              (dict(logits=torch.zeros((8, 40))), RuntimeError, "logits must be fp16"),
                              (dict(num_beams=0), ValueError, "num_beams=0"), (dict(num_beams=17), ValueError, "num_beams=17"),
                              (dict(num_beams=3), RuntimeError, "no multiple of num_beams=3"),
                              (dict(logits=torch.zeros((8, 7), dtype=torch.float16)), RuntimeError, "vocab=7"),
                              (dict(workspace=torch.zeros(127, dtype=torch.int32)), RuntimeError, "workspace must be int32"),
                              (dict(workspace=torch.zeros(128, dtype=torch.int64)), RuntimeError, "workspace must be int32")):
            with pytest.raises(err, match=msg):
                ops.beam_step(**dict(_step_args(), **bad))
        assert ops.copy_blocks(**_copy_args()) is None and ops.copy_blocks(**_copy_args(n=0)) is None
        for bad, err, msg in ((dict(pools=torch.zeros(4, dtype=torch.int32)), RuntimeError, "pools must be int64"),
                              (dict(src=torch.zeros(3, dtype=torch.int64)), RuntimeError, "src must be int32"),
                              (dict(dst=torch.zeros(2, dtype=torch.int32)), RuntimeError, "dst must be int32"),
                              (dict(block_bytes=24), ValueError, "block_bytes=24"), (dict(num_blocks=0), ValueError, "num_blocks=0")):
            with pytest.raises(err, match=msg):
                ops.copy_blocks(**dict(_copy_args(), **bad))


# ---- the reference of the step, on cases worked out by hand

def _row(vocab, **at):
    l = np.full(vocab, -10.0, np.float16)
    for t, v in at.items():
        l[int(t[1:])] = v
    return l


def test_reference_step_orders_by_score_then_beam_then_position():
    # B = 2, k = 4.  Two identical rows with identical cum: every score ties pairwise -> beam 0's candidate first, then beam 1's
    row = _row(16, t3=4.0, t5=3.0, t7=2.0, t9=1.0)
    out = beam_ref.beam_step(np.stack([row, row]), np.zeros(2, np.float32), np.ones(2, np.int32), 2, eos=-1)
    assert out["cand_token"].tolist() == [[3, 3, 5, 5]] and out["cand_parent"].tolist() == [[0, 1, 0, 1]]
    assert out["next_ids"].tolist() == [3, 3] and out["next_parent"].tolist() == [0, 1] and out["next_live"].tolist() == [1, 1]
    assert out["cand_score"][0, 0] == out["cand_logprob"][0, 0] == out["next_cum"][0]
    # a beam far behind drops out whole; eos inside the first B is left out of the next beams, which are the next two non-eos
    out = beam_ref.beam_step(np.stack([row, row]), np.array([0.0, -50.0], np.float32), np.ones(2, np.int32), 2, eos=5)
    assert out["cand_parent"].tolist() == [[0, 0, 0, 0]] and out["cand_token"].tolist() == [[3, 5, 7, 9]]
    assert out["next_ids"].tolist() == [3, 7] and out["next_parent"].tolist() == [0, 0]
    # eos outside the first B changes nothing of the next beams
    out = beam_ref.beam_step(np.stack([row, row]), np.array([0.0, -50.0], np.float32), np.ones(2, np.int32), 2, eos=9)
    assert out["next_ids"].tolist() == [3, 5]
    # a dead row contributes nothing; a prompt without a live row writes -1 / -inf and stays dead
    out = beam_ref.beam_step(np.stack([row, row, row, row]), np.zeros(4, np.float32), np.array([0, 1, 0, 0], np.int32), 2, eos=-1)
    assert out["cand_parent"].tolist() == [[1, 1, 1, 1], [-1, -1, -1, -1]] and out["cand_token"][1].tolist() == [-1] * 4
    assert np.isneginf(out["cand_score"][1]).all() and out["next_live"].tolist() == [1, 1, 0, 0] and out["next_parent"].tolist() == [1, 1, -1, -1]
    # more than 2B tokens tied at the cut: the lowest indices; fewer than 2B logits above -inf: the rest in index order at -inf, below everything
    tied = np.full(16, 1.0, np.float16)
    few = np.full(16, -np.inf, np.float16)
    few[[11, 2]] = [3.0, 3.0]
    out = beam_ref.beam_step(np.stack([tied, few]), np.zeros(2, np.float32), np.ones(2, np.int32), 2, eos=-1)
    assert out["cand_token"].tolist() == [[2, 11, 0, 1]] and out["cand_parent"].tolist() == [[1, 1, 0, 0]]
    lone = beam_ref.beam_step(few[None].repeat(2, 0), np.zeros(2, np.float32), np.array([0, 1], np.int32), 2, eos=-1)
    assert lone["cand_token"].tolist() == [[2, 11, 0, 1]] and np.isneginf(lone["cand_score"][0, 2:]).all()
    # a row without any logit above -inf: NaN values, ids 0 ... 2B - 1, equal to -inf in the order
    nothing = np.full(16, -np.inf, np.float16)
    out = beam_ref.beam_step(np.stack([nothing, few]), np.zeros(2, np.float32), np.ones(2, np.int32), 2, eos=-1)
    assert out["cand_token"].tolist() == [[2, 11, 0, 1]] and out["cand_parent"].tolist() == [[1, 1, 0, 0]] and np.isnan(out["cand_score"][0, 2:]).all()


# ---- PagedKVCache.reorder on CPU pools

BS = 16


def _cache(num_blocks=24, layers=2, dtype=torch.float16):
    from qqq_amd import PagedKVCache

    return PagedKVCache(layers, num_blocks, 2, 8, BS, dtype=dtype)


def _fill(cache, sid, n, mark):
    """a sequence of n keys whose every pool entry says (mark, position)"""
    cache.add(sid)
    step = cache.step([sid], [n])
    for pos, slot in zip(step.pos.tolist(), step.slots.tolist()):
        blk, off = divmod(slot, BS)
        for pool in cache.k + cache.v:
            pool[blk, :, off, :] = (mark * 40 + pos) % 127
        if cache.quantized:
            for pool in cache.k_scale + cache.v_scale:
                pool[blk, :, off] = mark * 1000 + pos


def _content(cache, sid):
    n = cache.length(sid)
    idx = [b * BS + o for b in cache.blocks(sid) for o in range(BS)][:n]
    out = []
    for pool in cache._pools()[0]:
        out.append(pool.transpose(1, 2).reshape(cache.num_blocks * BS, -1)[idx].clone())
    for pool in cache._pools()[1]:
        out.append(pool.transpose(1, 2).reshape(cache.num_blocks * BS, -1)[idx].clone())
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
@pytest.mark.parametrize("n", [32, 37, 5])
def test_reorder_identity_and_permutation_take_no_block_and_copy_nothing(n, dtype):
    cache = _cache(dtype=dtype)
    for s in range(3):
        _fill(cache, s, n, s + 1)
    free, blocks, was = cache.free_blocks, [cache.blocks(s) for s in range(3)], [_content(cache, s) for s in range(3)]
    cache.reorder([0, 1, 2], [0, 1, 2])
    assert [cache.blocks(s) for s in range(3)] == blocks and cache.free_blocks == free
    cache.reorder([0, 1, 2], [2, 0, 1])
    assert [cache.blocks(s) for s in range(3)] == [blocks[2], blocks[0], blocks[1]] and cache.free_blocks == free
    assert all(_same(_content(cache, s), was[p]) for s, p in zip(range(3), (2, 0, 1)))
    assert all(cache._refs[b] == 1 for s in range(3) for b in cache.blocks(s)) and all(cache.shared_keys(s) == 0 for s in range(3))
    for s in range(3):
        cache.free(s)
    assert cache.free_blocks == 24


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
@pytest.mark.parametrize("n", [32, 37, 5, 16])
def test_reorder_one_parent_taken_by_all(n, dtype):
    cache = _cache(dtype=dtype)
    for s in range(4):
        _fill(cache, s, n, s + 1)
    cache.add("other")
    _fill(cache, "foreign", 20, 9)
    foreign, foreign_blocks = _content(cache, "foreign"), cache.blocks("foreign")
    full, part = n // BS, n % BS != 0
    want, parent_blocks = _content(cache, 2), cache.blocks(2)
    released = 3 * (-(-n // BS))
    free = cache.free_blocks
    cache.reorder([0, 1, 2, 3], [2, 2, 2, 2])
    assert cache.free_blocks == free + released - (3 if part else 0)  # the unchosen free theirs, exactly m - 1 fresh blocks are taken
    assert cache.blocks(0) == parent_blocks  # the first taker gets the parent's blocks, no copy
    for s in range(4):
        assert cache.length(s) == n and _same(_content(cache, s), want)
        assert cache.blocks(s)[:full] == parent_blocks[:full] and cache.shared_keys(s) == full * BS
        assert cache.root(s) is cache.root(0) and cache.root(s) not in (0, 1, 2, 3)
    assert all(cache._refs[b] == 4 for b in parent_blocks[:full])
    if part:
        last = [cache.blocks(s)[full] for s in range(4)]
        assert len(set(last)) == 4 and all(cache._refs[b] == 1 for b in last)
    assert _same(_content(cache, "foreign"), foreign) and cache.blocks("foreign") == foreign_blocks and cache.root("foreign") == "foreign"
    # the siblings are a family for the next decode step, and go their own ways from here
    step = cache.step([0, 1, 2, 3], [1, 1, 1, 1])
    if full:
        assert step.family.tolist() == [0, 0, 0, 0] and step.shared.tolist() == [full * BS] * 4 and step.family_max == 4
    assert len({cache.blocks(s)[-1] for s in range(4)}) == 4
    # two parents: what all four have in common is what the two parents had
    cache.reorder([0, 1, 2, 3], [0, 0, 3, 3])
    assert [cache.shared_keys(s) for s in range(4)] == [full * BS] * 4
    for s in (0, 1, 2, 3, "other", "foreign"):
        cache.free(s)
    assert cache.free_blocks == 24 and all(r == 0 for r in cache._refs)


def test_reorder_admits_new_sequences_and_keeps_families_apart():
    cache = _cache()
    _fill(cache, "a0", 21, 1)
    _fill(cache, "b0", 21, 2)
    a, b = _content(cache, "a0"), _content(cache, "b0")
    cache.reorder(["a0", "a1", "a2", "b0", "b1", "b2"], [0, 0, 0, 3, 3, 3])  # the first pass behind a prefill: beam 0 alone exists
    assert all(_same(_content(cache, s), a) for s in ("a0", "a1", "a2")) and all(_same(_content(cache, s), b) for s in ("b0", "b1", "b2"))
    assert cache.root("a1") is cache.root("a0") and cache.root("b2") is cache.root("b0") and cache.root("a0") is not cache.root("b0")
    step = cache.step(["a0", "a1", "a2", "b0", "b1", "b2"], [1] * 6)
    assert step.family.tolist() == [0, 0, 0, 3, 3, 3] and step.shared.tolist() == [16] * 6
    with pytest.raises(KeyError, match="no sequence"):
        cache.reorder(["a0", "new", "newer"], [0, 2, 0])  # a sequence the call admits cannot be a parent
    for s in ("a0", "a1", "a2", "b0", "b1", "b2"):
        cache.free(s)
    assert cache.free_blocks == 24


def test_reorder_refuses_and_changes_nothing():
    cache = _cache(num_blocks=7)
    for s in range(3):
        _fill(cache, s, 21, s + 1)  # 6 blocks, 1 free
    state = lambda: ([cache.blocks(s) for s in range(3)], list(cache._free), list(cache._refs), [cache.root(s) for s in range(3)])  # noqa: E731
    before = state()
    cache.add(3)
    with pytest.raises(RuntimeError, match=r"reorder: the pool is exhausted \(3 blocks needed, 1 free\)"):
        cache.reorder([0, 1, 2, "x", "y", "z"], [0, 0, 1, 1, 2, 2])
    with pytest.raises(ValueError, match="index into"):
        cache.reorder([0, 1], [0, 2])
    with pytest.raises(ValueError, match="without repeated"):
        cache.reorder([0, 0], [0, 0])
    with pytest.raises(ValueError, match="non-empty"):
        cache.reorder([], [])
    assert state() == before
    # ... while the blocks the unchosen release count: 0 taken three times needs two fresh blocks, one is free and four come back
    cache.reorder([0, 1, 2], [0, 0, 0])
    assert cache.free_blocks == 3 and cache.length(2) == 21 and cache._refs[cache.blocks(0)[0]] == 3
    for s in range(4):
        cache.free(s)
    assert cache.free_blocks == 7


# ---- beam_search over a stub model: the forward pass writes its tokens into the (CPU) key pool and derives every row's logits from what the
# sequence's blocks hold, so a reorder that pointed a beam at the wrong blocks would change the search

VOCAB, EOS = 50, 7


def _logits_of(tokens):
    """a row of fp16 logits for a sequence: pseudo-random in the whole history, a few large values so that beams compete, eos now and then"""
    h = 1469598103
    for t in tokens:
        h = (h * 1099511 + int(t) + 1) % 2147483647
    rng = np.random.default_rng(h)
    row = rng.standard_normal(VOCAB).astype(np.float32)
    row[rng.integers(0, VOCAB, 3)] += rng.random(3).astype(np.float32) * 4
    if h % 3 == 0:
        row[EOS] += 5.0
    return row.astype(np.float16)


class _Stub:
    def __init__(self, lm, monkeypatch):
        self.passes, self.rows, self.reorders = [], [], 0
        monkeypatch.setattr(lm, "forward", self.forward)
        monkeypatch.setattr("qqq_amd.beam.ops.beam_step", self.step)
        monkeypatch.setattr("qqq_amd.model.ops.sample_tokens", lambda logits, T, k, p, u: logits.argmax(dim=1))

    def forward(self, ids, cache, step, all_rows=False):
        assert ids.dtype == torch.int64 and ids.shape == (sum(step.counts),)
        cache.k[0][step.slots // cache.block_size, 0, step.slots % cache.block_size, 0] = ids.to(cache.k[0].dtype)
        flat = cache.k[0][:, 0, :, 0].reshape(-1)  # [num_blocks * block_size]: head 0, element 0 of every key
        self.passes.append("decode" if step.decode and len(ids) == len(step.seq_ids) and step.counts[0] == 1 and step.starts[0] else "prefill")
        self.rows.append(len(step.seq_ids))
        out = []
        for sid in step.seq_ids:
            bs = cache.block_size
            idx = [b * bs + o for b in cache.blocks(sid) for o in range(bs)][:cache.length(sid)]
            out.append(_logits_of(flat[idx].long().tolist()))
        return torch.from_numpy(np.stack(out))

    def step(self, logits, cum, live, num_beams, eos=None, workspace=None):
        from qqq_amd import ops

        assert workspace is not None and workspace.dtype == torch.int32 and workspace.shape[0] >= 4 * logits.shape[0] * num_beams
        o = beam_ref.beam_step(logits.numpy(), cum.numpy(), live.numpy(), num_beams, -1 if eos is None else eos)
        t = {k: torch.from_numpy(v) for k, v in o.items()}
        packed = torch.cat([t["cand_score"].reshape(-1).view(torch.int32), t["cand_logprob"].reshape(-1).view(torch.int32),
                            t["cand_parent"].reshape(-1), t["cand_token"].reshape(-1), t["next_parent"]])
        return ops.BeamStep(t["cand_score"], t["cand_logprob"], t["cand_parent"], t["cand_token"], t["next_ids"], t["next_parent"],
                            t["next_cum"], t["next_live"], packed)


def _lm(monkeypatch):
    from test_step_cpu import _tiny_lm

    lm = _tiny_lm()
    return lm, _Stub(lm, monkeypatch)


def _reference(prompts, T, B, **kw):
    return [beam_ref.search(_logits_of, p, T, B, **kw) for p in prompts]


def _as_tuples(results):
    return [[(list(h.tokens), h.score, h.logprob) for h in r] for r in results]


PROMPTS = [[3, 9, 4], list(range(10, 27)), [5] * 16, [1, 2]]


@pytest.mark.parametrize("B, T, early, lp, nret", [(4, 9, False, 1.0, 4), (4, 9, True, 1.0, 2), (3, 20, False, 2.0, 3), (2, 18, False, 0.0, 1),
                                                    (5, 6, True, 0.0, 5), (1, 12, False, 1.0, 1), (16, 4, False, 1.0, 16)])
def test_beam_search_equals_the_reference_search(monkeypatch, B, T, early, lp, nret):
    lm, stub = _lm(monkeypatch)
    cache = lm.new_cache(200)
    got = lm.beam_search(PROMPTS, T, num_beams=B, length_penalty=lp, early_stopping=early, eos_token_id=EOS, num_return_sequences=nret,
                         cache=cache)
    want = _reference(PROMPTS, T, B, length_penalty=lp, early_stopping=early, eos=EOS, num_return=nret)
    assert _as_tuples(got) == want
    assert all(len(r) == nret and isinstance(h, type(got[0][0])) for r in got for h in r)
    assert all(r[i].score >= r[i + 1].score for r in got for i in range(len(r) - 1))
    assert all(h.score == h.logprob / len(h.tokens) ** lp for r in got for h in r)
    assert cache.free_blocks == 200 and stub.passes[0] == "prefill" and stub.rows[0] == len(PROMPTS)
    assert all(rows % B == 0 for rows in stub.rows[1:])  # every later pass runs all beams of the running prompts


def test_beam_search_without_eos_runs_to_the_budget(monkeypatch):
    lm, stub = _lm(monkeypatch)
    got = lm.beam_search(PROMPTS[:2], 5, num_beams=3, num_return_sequences=3)
    assert _as_tuples(got) == _reference(PROMPTS[:2], 5, 3, num_return=3)
    assert all(len(h.tokens) == 5 for r in got for h in r) and stub.rows == [2, 6, 6, 6, 6]


def test_one_beam_is_greedy_generate(monkeypatch):
    lm, _ = _lm(monkeypatch)
    for eos in (EOS, None):
        greedy = lm.generate(PROMPTS, 14, eos_token_id=eos)
        beams = lm.beam_search(PROMPTS, 14, num_beams=1, eos_token_id=eos)
        assert [r[0].tokens for r in beams] == greedy
    assert any(g[-1] == EOS and len(g) < 14 for g in lm.generate(PROMPTS, 14, eos_token_id=EOS))  # the case has an early end in it


def _scripted(lm, monkeypatch, rows_by_pass):
    """forward: every row of pass i (the last one for good) holds rows_by_pass[i]'s logits and -20 elsewhere -> the rows of each pass"""
    calls = []

    def forward(ids, cache, step, all_rows=False):
        calls.append(len(step.seq_ids))
        spec = rows_by_pass[min(len(calls), len(rows_by_pass)) - 1]
        row = np.full(VOCAB, -20.0 if spec else 0.0, np.float16)
        for t, v in spec.items():
            row[t] = v
        return torch.from_numpy(np.stack([row] * len(step.seq_ids)))

    monkeypatch.setattr(lm, "forward", forward)
    return calls


def test_eos_counts_only_among_the_first_num_beams_candidates(monkeypatch):
    """B = 2, score = logprob (length_penalty 0).  Pass 1 makes the beams [11] and [12], two nats apart.  Pass 2 puts beam 0's eos at
    position 2 of the four candidates (behind 21 and 22 of beam 0) or at position 1; pass 3 is a flat row (every token -log 50), so a
    hypothesis [11, eos] held at pass 2 beats whatever is live at the budget -- if it was held."""
    lm, _ = _lm(monkeypatch)
    first = {11: 6.0, 12: 4.0, 13: 3.0, 14: 2.0}
    calls = _scripted(lm, monkeypatch, [first, {21: 6.0, 22: 5.0, EOS: 4.0, 23: 3.0}, {}])
    got = lm.beam_search([[1, 2, 3]], 3, num_beams=2, length_penalty=0.0, eos_token_id=EOS, num_return_sequences=2)[0]
    assert [h.tokens for h in got] == [[11, 21, 0], [11, 21, 1]] and calls == [1, 2, 2]  # position 2 >= B: no hypothesis
    calls = _scripted(lm, monkeypatch, [first, {21: 6.0, EOS: 5.5, 22: 3.0, 23: 2.0}, {}])
    got = lm.beam_search([[1, 2, 3]], 3, num_beams=2, length_penalty=0.0, eos_token_id=EOS, num_return_sequences=2)[0]
    assert [h.tokens for h in got] == [[11, EOS], [11, 21, 0]] and calls == [1, 2, 2]       # position 1 < B: held, with its eos
    assert got[0].score == got[0].logprob > got[1].logprob
    calls = _scripted(lm, monkeypatch, [{EOS: 7.0, 11: 6.0, 12: 4.0, 13: 3.0}])
    got = lm.beam_search([[1, 2, 3]], 1, num_beams=2, eos_token_id=EOS, num_return_sequences=2)[0]
    assert [h.tokens for h in got] == [[EOS], [11]] and calls == [1]  # at the budget the live beams finish as they are; B are kept


def test_early_stopping_ends_a_prompt_once_num_beams_are_held(monkeypatch):
    """Every row: eos 6, 11 5, 12 3 -> log-probabilities about -0.35, -1.35, -3.35.  Pass 1 holds [eos] (-0.35), beams [11], [12].  Pass 2:
    (0, eos) -1.70 at position 0 is held, (0, 11) -2.70, (1, eos) -3.70 at position 2 is not, (0, 12) -4.70: two are held."""
    lm, _ = _lm(monkeypatch)
    row = {EOS: 6.0, 11: 5.0, 12: 3.0}
    calls = _scripted(lm, monkeypatch, [row])
    early = lm.beam_search([[1, 2]], 30, num_beams=2, early_stopping=True, eos_token_id=EOS, num_return_sequences=2, length_penalty=3.0)[0]
    assert calls == [1, 2] and [h.tokens for h in early] == [[11, EOS], [EOS]]  # -1.70 / 2 ** 3 is above -0.35 / 1
    # the heuristic with score = logprob: the best live beam (-2.70) is not above the worst held (-1.70) -> the same end
    calls = _scripted(lm, monkeypatch, [row])
    late = lm.beam_search([[1, 2]], 30, num_beams=2, early_stopping=False, eos_token_id=EOS, num_return_sequences=2, length_penalty=0.0)[0]
    assert calls == [1, 2] and [h.tokens for h in late] == [[EOS], [11, EOS]]
    # ... with length_penalty 3 the live beam's -2.70 / 8 is above the worst held -0.35: the prompt goes on
    calls = _scripted(lm, monkeypatch, [row])
    lm.beam_search([[1, 2]], 30, num_beams=2, early_stopping=False, eos_token_id=EOS, num_return_sequences=2, length_penalty=3.0)
    assert len(calls) > 2


@pytest.mark.parametrize("lp", [0.0, 1.0, 2.0])
def test_length_penalty_orders_the_hypotheses(monkeypatch, lp):
    lm, _ = _lm(monkeypatch)
    res = lm.beam_search(PROMPTS[:2], 12, num_beams=4, length_penalty=lp, eos_token_id=EOS, num_return_sequences=4, early_stopping=True)
    for r in res:
        assert [h.score for h in r] == sorted((h.logprob / len(h.tokens) ** lp for h in r), reverse=True)
        assert lp or r[0].logprob == max(h.logprob for h in r)
    assert len({len(h.tokens) for r in res for h in r}) > 1  # hypotheses of several lengths: the penalty had something to order


def test_admission_formula_waiting_in_order_and_a_prompt_that_never_fits(monkeypatch):
    from qqq_amd import beam

    assert beam.blocks_needed(3, 9, 4, 16) == 4 and beam.blocks_needed(17, 9, 4, 16) == 2 + 3 * 1 and beam.blocks_needed(16, 17, 4, 16) == 2 + 3
    assert beam.blocks_needed(40, 30, 1, 16) == 5 and beam.blocks_needed(33, 1, 16, 16) == 3 + 15
    lm, stub = _lm(monkeypatch)
    T, B = 9, 4
    need = [beam.blocks_needed(len(p), T, B, 16) for p in PROMPTS]
    want = _reference(PROMPTS, T, B, eos=EOS)
    # a pool for the largest prompt alone: one prompt at a time, in order, the same hypotheses; the pool is never asked for more
    cache = lm.new_cache(max(need))
    low = [cache.free_blocks]
    take = cache._take
    monkeypatch.setattr(cache, "_take", lambda: (low.append(cache.free_blocks - 1), take())[1])
    assert _as_tuples(lm.beam_search(PROMPTS, T, num_beams=B, eos_token_id=EOS, cache=cache)) == want
    assert [r for r, p in zip(stub.rows, stub.passes) if p == "prefill"] == [1, 1, 1, 1] and min(low) >= 0 and cache.free_blocks == max(need)
    # room for the first two together: they are prefilled in one pass, the others wait
    lm, stub = _lm(monkeypatch)
    cache = lm.new_cache(need[0] + need[1])
    assert _as_tuples(lm.beam_search(PROMPTS, T, num_beams=B, eos_token_id=EOS, cache=cache)) == want
    assert stub.rows[0] == 2 and cache.free_blocks == need[0] + need[1]
    # a foreign sequence in the pool is left alone, and what it holds is not counted as free
    cache = lm.new_cache(max(need) + 2)
    cache.add("foreign")
    cache.step(["foreign"], [20])
    mine = cache.blocks("foreign")
    assert _as_tuples(lm.beam_search(PROMPTS, T, num_beams=B, eos_token_id=EOS, cache=cache)) == want
    assert cache.blocks("foreign") == mine and cache.length("foreign") == 20 and cache.free_blocks == max(need)
    # one block short of the largest prompt: it can never fit; the pool is left as it was found
    cache = lm.new_cache(max(need) - 1)
    with pytest.raises(RuntimeError, match="cannot hold a prompt"):
        lm.beam_search(PROMPTS, T, num_beams=B, eos_token_id=EOS, cache=cache)
    assert cache.free_blocks == max(need) - 1


def test_beam_search_refuses_bad_keywords(monkeypatch):
    lm, _ = _lm(monkeypatch)
    for kw, msg in ((dict(num_beams=0), "num_beams=0"), (dict(num_beams=17), "num_beams=17"), (dict(num_beams=4, num_return_sequences=5), "num_return_sequences=5"),
                    (dict(num_return_sequences=0), "num_return_sequences=0"), (dict(eos_token_id=50), "eos_token_id=50")):
        with pytest.raises(ValueError, match=msg):
            lm.beam_search(PROMPTS, 4, **kw)
    with pytest.raises(ValueError, match="at least one token"):
        lm.beam_search([[1], []], 4)
    for kw in ("temperature", "stop", "logprobs", "device_loop", "draft_len", "n", "repetition_penalty"):
        with pytest.raises(TypeError):
            lm.beam_search(PROMPTS, 4, **{kw: 1})
    assert lm.beam_search(PROMPTS, 0) == [[], [], [], []] and lm.beam_search([], 4) == []
