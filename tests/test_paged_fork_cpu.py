"""PagedKVCache.fork and the reference counts behind it, on CPU tensors: which blocks a fork shares and which it copies, what free()
returns and when, that sequences which never fork see the allocator they always saw, and the family fields of a PagedStep."""
import pytest
import torch

from qqq_amd.paged import PagedKVCache


def _cache(num_blocks=12, block_size=16, dtype=torch.float16, layers=2, kvh=2, d=64):
    return PagedKVCache(layers, num_blocks, kvh, d, block_size, device="cpu", dtype=dtype)


def _fill(cache, seed=0):
    """every pool row distinct, so a copy that took the wrong block or layer shows"""
    g = torch.Generator().manual_seed(seed)
    for layer in range(cache.num_layers):
        for pool in (cache.k[layer], cache.v[layer]):
            if cache.quantized:
                pool.copy_(torch.randint(-127, 128, pool.shape, generator=g, dtype=torch.int8))
            else:
                pool.copy_(torch.randn(pool.shape, generator=g).half())
        if cache.quantized:
            for sc in (cache.k_scale[layer], cache.v_scale[layer]):
                sc.copy_(torch.rand(sc.shape, generator=g) + 0.01)


def _state(cache):
    return (cache.free_blocks, list(cache._free), list(cache._refs), {s: list(b) for s, b in cache._blocks.items()}, dict(cache._len))


@pytest.mark.parametrize("length, full, fresh", [(5, 0, 1), (16, 1, 0), (37, 2, 1), (48, 3, 0)])
def test_fork_shares_exactly_the_full_blocks(length, full, fresh):
    cache = _cache()
    cache.add("a")
    cache.step(["a"], [length])
    before = cache.free_blocks
    cache.fork("a", "b")
    a, b = cache.blocks("a"), cache.blocks("b")
    assert b[:full] == a[:full] and len(b) == full + fresh
    assert cache.free_blocks == before - fresh
    assert cache.length("b") == length
    if fresh:
        assert b[full] not in a  # the partial block is the fork's own
    assert cache.shared_keys("b") == full * 16 and cache.shared_keys("a") == full * 16
    assert cache.root("b") == "a" and cache.root("a") == "a"


def test_fork_leaves_reserved_blocks_with_the_source():
    cache = _cache()
    cache.add("a")
    cache.reserve("a", 100)  # 7 blocks
    cache.step(["a"], [20])
    cache.fork("a", "b")
    assert len(cache.blocks("a")) == 7 and len(cache.blocks("b")) == 2
    assert cache.blocks("b")[0] == cache.blocks("a")[0] and cache.blocks("b")[1] not in cache.blocks("a")


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
@pytest.mark.parametrize("length", [5, 37])
def test_fork_copies_the_partial_block_in_every_layer(dtype, length):
    cache = _cache(dtype=dtype)
    _fill(cache)
    cache.add("a")
    cache.step(["a"], [length])
    cache.fork("a", "b")
    for layer in range(cache.num_layers):
        for x, y in zip(cache.gather(layer, "a"), cache.gather(layer, "b")):
            assert torch.equal(x, y)
        new, old = cache.blocks("b")[-1], cache.blocks("a")[length // 16]
        assert torch.equal(cache.k[layer][new], cache.k[layer][old]) and torch.equal(cache.v[layer][new], cache.v[layer][old])
        if cache.quantized:
            assert torch.equal(cache.k_scale[layer][new], cache.k_scale[layer][old])
            assert torch.equal(cache.v_scale[layer][new], cache.v_scale[layer][old])


@pytest.mark.parametrize("first", ["a", "b"])
def test_free_blocks_through_fork_step_and_free(first):
    cache = _cache(num_blocks=10)
    cache.add("a")
    cache.step(["a"], [37])  # 3 blocks: two full, one partial
    assert cache.free_blocks == 7
    cache.fork("a", "b")  # one fresh block
    assert cache.free_blocks == 6
    shared = cache.blocks("a")[:2]
    cache.step(["a", "b"], [1, 1])  # 38 keys: inside the partial blocks
    assert cache.free_blocks == 6
    cache.step(["a", "b"], [11, 11])  # 49 keys: a fourth block each
    assert cache.free_blocks == 4
    second = "b" if first == "a" else "a"
    cache.free(first)  # its two own blocks come back, the shared ones stay with the other owner
    assert cache.free_blocks == 6
    assert not set(shared) & set(cache._free)
    assert cache.blocks(second)[:2] == shared
    cache.free(second)
    assert cache.free_blocks == 10 and sorted(cache._free) == list(range(10))
    assert all(r == 0 for r in cache._refs)


def test_three_owners_return_a_shared_block_with_the_last():
    cache = _cache(num_blocks=8)
    cache.add("a")
    cache.step(["a"], [16])
    cache.fork("a", "b")
    cache.fork("a", "c")
    blk = cache.blocks("a")[0]
    assert cache.blocks("b") == [blk] and cache.blocks("c") == [blk] and cache.free_blocks == 7
    cache.free("a")
    cache.free("c")
    assert cache.free_blocks == 7 and blk not in cache._free
    cache.free("b")
    assert cache.free_blocks == 8 and cache._free[-1] == blk


def test_sequences_that_never_fork_see_the_same_block_ids():
    """The stack discipline of the allocator, restated: block 0 goes out first, a freed sequence's blocks go back in the order it took
    them, so the last one it took is the next one out."""
    cache = _cache(num_blocks=8)
    cache.add("a")
    cache.add("b")
    cache.step(["a", "b"], [17, 5])
    assert cache.blocks("a") == [0, 1] and cache.blocks("b") == [2]
    cache.step(["b", "a"], [12, 16])  # b: 17 keys, a: 33 keys
    assert cache.blocks("b") == [2, 3] and cache.blocks("a") == [0, 1, 4]
    cache.free("a")  # 0, 1, 4 go back: 4 is the next one out, then 1, then 0
    cache.add("c")
    cache.step(["c"], [40])
    assert cache.blocks("c") == [4, 1, 0]
    cache.reserve("b", 50)
    assert cache.blocks("b") == [2, 3, 5, 6]
    cache.free("c")
    cache.free("b")
    cache.add("d")
    cache.step(["d"], [1])
    assert cache.blocks("d") == [6]
    assert cache.free_blocks == 7


def test_steps_after_a_fork_write_to_distinct_slots():
    cache = _cache()
    cache.add("a")
    cache.step(["a"], [37])
    cache.fork("a", "b")
    st = cache.step(["a", "b"], [1, 1])
    slots = st.slots.tolist()
    assert slots[0] != slots[1]
    assert slots[0] // 16 == cache.blocks("a")[2] and slots[1] // 16 == cache.blocks("b")[2] and slots[0] % 16 == slots[1] % 16 == 37 % 16
    shared = set(cache.blocks("a")[:2])
    assert not {s // 16 for s in slots} & shared
    # at a block boundary both take a block of their own
    cache2 = _cache()
    cache2.add("a")
    cache2.step(["a"], [32])
    cache2.fork("a", "b")
    st = cache2.step(["a", "b"], [1, 1])
    blocks = [s // 16 for s in st.slots.tolist()]
    assert blocks[0] != blocks[1] and not set(blocks) & set(cache2.blocks("a")[:2])
    assert st.block_table[:, :2].tolist() == [cache2.blocks("a")[:2]] * 2


def test_fork_raises_and_changes_nothing():
    cache = _cache(num_blocks=3)
    cache.add("a")
    cache.step(["a"], [37])  # the pool is used up
    cache.add("c")
    before = _state(cache)
    with pytest.raises(RuntimeError, match="exhausted"):
        cache.fork("a", "b")
    assert _state(cache) == before
    with pytest.raises(KeyError):
        cache.fork("a", "c")  # dst exists
    assert _state(cache) == before
    with pytest.raises(KeyError):
        cache.fork("nobody", "b")
    assert _state(cache) == before
    full = _cache(num_blocks=2)
    full.add("a")
    full.step(["a"], [32])
    full.fork("a", "b")  # no block needed: an exhausted pool still forks at a block boundary
    assert full.blocks("b") == full.blocks("a") and full.free_blocks == 0


def test_paged_step_family_fields():
    cache = _cache(num_blocks=64)
    for name, n in (("p", 40), ("q", 20), ("r", 70)):
        cache.add(name)
        cache.step([name], [n])
    cache.fork("p", "p1")  # shares 32 keys
    cache.fork("p", "p2")
    cache.fork("r", "r1")  # shares 64 keys
    cache.step(["r"], [26])  # r: 96 keys
    cache.fork("r", "r2")  # shares 96 keys with r, but r1 only 64: the family's minimum
    st = cache.step(["p", "p1", "p2", "q", "r", "r1", "r2"], [1] * 7)
    assert st.family.dtype == torch.int32 and st.shared.dtype == torch.int64
    assert st.family.tolist() == [0, 0, 0, 3, 4, 4, 4]
    assert st.shared.tolist() == [32, 32, 32, 0, 64, 64, 64]
    assert st.family_max == 3
    # two of a family next to each other share what the two share
    st = cache.step(["r", "r2", "q"], [1, 1, 1])
    assert st.family.tolist() == [0, 0, 2] and st.shared.tolist() == [96, 96, 0] and st.family_max == 2
    # siblings that are not adjacent are lone rows; a step without adjacent siblings has no family fields
    st = cache.step(["p", "q", "p1"], [1, 1, 1])
    assert st.family is None and st.shared is None and st.family_max is None
    st = cache.step(["q"], [1])
    assert st.family is None
    # a prefill step (more than one token somewhere) never has them
    st = cache.step(["p", "p1"], [2, 1])
    assert st.family is None and st.shared is None and st.family_max is None
    # a freed root leaves its family a family
    cache.free("p")
    st = cache.step(["p1", "p2"], [1, 1])
    assert st.family.tolist() == [0, 0] and st.shared.tolist() == [32, 32]
