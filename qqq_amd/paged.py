"""The block-table (paged) KV cache: per layer a pool of blocks of `block_size` keys that any sequence may own, a host-side block allocator
with per-sequence lengths, and the per-step metadata the paged ops read (ops.rope_qkv_paged / decode_attention_paged /
prefill_attention_paged and their _kv8 forms).

    PagedKVCache   k[layer], v[layer] of shape [num_blocks, num_kv_heads, block_size, head_dim] (fp16 or int8; an int8 pool with
                   k_scale[layer], v_scale[layer] [num_blocks, num_kv_heads, block_size]); add / fork / reorder / free / reserve / step /
                   advance / gather
    PagedStep      what one forward pass over a packed batch of sequences needs, built once on the host and shared by all layers

Sequences arrive and finish at different times, have different lengths, and a finished sequence's blocks serve the next one.  The allocator
counts the owners of every block: fork() makes a sequence that shares the full blocks of another one (the n completions of one prompt),
and a shared block returns to the free list with its last owner.  Only full blocks are shared, so no write ever lands in one.
reorder() re-points a group of sequences at one another's blocks by the same rules (the beams of a beam search, every pass).  The
sequences forked from one prompt are a family; a decode step over adjacent siblings says so in PagedStep.family / shared / family_max,
which ops.decode_attention_paged_shared reads.  The ops themselves need none of this: a block table may name any block.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch


@dataclass
class PagedStep:
    """One step of a packed batch: sequence i contributes counts[i] tokens at positions starts[i] ... starts[i] + counts[i] - 1, in order.

    Host fields: seq_ids, counts, starts, max_len (the longest sequence after the step), decode (every count is 1).
    Device tensors: pos int64 [m] and slots int64 [m] per token (m = sum(counts)); block_table int32 [b, W] (row i: the blocks of
    sequence i, padded with 0) and last_pos int64 [b] (the position of each sequence's last token) per sequence; cu_tokens int32 [b + 1]
    (sequence i owns tokens cu_tokens[i] ... cu_tokens[i + 1] - 1 of the packed batch) and start_pos int64 [b] (= starts), which
    ops.prefill_attention_paged reads.
    Families (None unless the step is a decode step in which at least two adjacent sequences were forked from one prompt): family int32
    [b] (the index within the step of the first row of row i's family; a lone row names itself), shared int64 [b] (the leading keys a row
    has in common with its family -- a multiple of the block size, the family's minimum, the same on all its rows; 0 for a lone row) and
    family_max (host: the largest family of the step).
    lora (None: no adapters, and then nothing of it runs): a LoraStep (qqq_amd/lora.py) -- the bank and token_slot int32 [m] on the device,
    the adapter slot of every token of the step, -1 for none."""
    seq_ids: List
    counts: List[int]
    starts: List[int]
    max_len: int
    decode: bool
    pos: torch.Tensor
    slots: torch.Tensor
    block_table: torch.Tensor
    last_pos: torch.Tensor
    cu_tokens: Optional[torch.Tensor] = None
    start_pos: Optional[torch.Tensor] = None
    family: Optional[torch.Tensor] = None
    shared: Optional[torch.Tensor] = None
    family_max: Optional[int] = None
    lora: Optional[object] = None


class _Family:
    """The root of a family PagedKVCache.reorder() formed: equal to itself alone, and no sequence id."""
    __slots__ = ()

    def __repr__(self):
        return f"<family {id(self):#x}>"


class PagedKVCache:
    """Key / value block pools of `num_layers` layers and the allocator of their blocks (one block id covers all layers).

    dtype=torch.float16 (default): fp16 K and V, 4 * num_layers * num_blocks * num_kv_heads * block_size * head_dim bytes.
    dtype=torch.int8: every head row is dynamic_quant of that fp16 row, as in KVCache(dtype=torch.int8):
    2 * num_layers * num_blocks * num_kv_heads * block_size * (head_dim + 4) bytes.  Any other dtype raises.
    block_size is a power of two in [16, 256]."""

    def __init__(self, num_layers: int, num_blocks: int, num_kv_heads: int, head_dim: int, block_size: int, device=None,
                 dtype=torch.float16):
        if dtype not in (torch.float16, torch.int8):
            raise ValueError(f"PagedKVCache: dtype must be torch.float16 or torch.int8, not {dtype}")
        if block_size not in (16, 32, 64, 128, 256):
            raise ValueError(f"PagedKVCache: block_size must be a power of two in [16, 256], not {block_size}")
        if num_blocks < 1:
            raise ValueError(f"PagedKVCache: num_blocks must be at least 1, not {num_blocks}")
        self.num_layers, self.num_blocks, self.num_kv_heads, self.head_dim, self.block_size = (num_layers, num_blocks, num_kv_heads,
                                                                                               head_dim, block_size)
        self.dtype, self.device = dtype, device
        shape = (num_blocks, num_kv_heads, block_size, head_dim)
        self.k = [torch.zeros(shape, dtype=dtype, device=device) for _ in range(num_layers)]
        self.v = [torch.zeros(shape, dtype=dtype, device=device) for _ in range(num_layers)]
        if dtype == torch.int8:
            self.k_scale = [torch.zeros(shape[:3], dtype=torch.float32, device=device) for _ in range(num_layers)]
            self.v_scale = [torch.zeros(shape[:3], dtype=torch.float32, device=device) for _ in range(num_layers)]
        self._free: List[int] = list(range(num_blocks - 1, -1, -1))  # a stack: block 0 goes out first, a freed block is the next one out
        self._blocks: Dict[object, List[int]] = {}
        self._len: Dict[object, int] = {}
        self._refs: List[int] = [0] * num_blocks  # owners of a block: 0 on the free list, above 1 only for full blocks that fork() shared
        self._root: Dict[object, object] = {}     # the sequence a family was forked from (a sequence that never forked names itself)
        self._shared: Dict[object, int] = {}      # leading keys in common with the family: what fork() shared, a multiple of block_size
        self._tables = None                       # reorder()'s pointer tables of the pools (GPU pools only), built at its first copy

    @property
    def quantized(self) -> bool:
        return self.dtype == torch.int8

    @property
    def nbytes(self) -> int:
        rows = self.num_layers * self.num_blocks * self.num_kv_heads * self.block_size
        return 2 * rows * (self.head_dim + 4) if self.quantized else 4 * rows * self.head_dim

    @property
    def capacity(self) -> int:
        """The longest sequence the pool could hold (all blocks to one sequence): what the rope tables are sized for."""
        return self.num_blocks * self.block_size

    # ---- the allocator (host only)

    @property
    def free_blocks(self) -> int:
        return len(self._free)

    def add(self, seq_id) -> None:
        """Admit an empty sequence; it owns no block until its first step()."""
        if seq_id in self._blocks:
            raise KeyError(f"PagedKVCache.add: sequence {seq_id!r} exists")
        self._blocks[seq_id], self._len[seq_id] = [], 0
        self._root[seq_id], self._shared[seq_id] = seq_id, 0

    def _take(self) -> int:
        blk = self._free.pop()
        self._refs[blk] = 1
        return blk

    def fork(self, src, dst) -> None:
        """Admit `dst` as a copy of `src` at its present length: it shares src's len // block_size full blocks (one more owner each) and,
        where the length is no multiple of block_size, takes one fresh block that receives a copy of src's partial block in every layer
        (k, v and an int8 pool's scales).  Blocks src has reserved beyond its length stay src's alone.  dst joins src's family, with
        shared_keys() the full blocks' keys (for a fork of a fork, no more than its source shares with the root).  Raises, and changes
        nothing, if dst exists or src does not (KeyError) or the pool cannot supply the block (RuntimeError)."""
        if dst in self._blocks:
            raise KeyError(f"PagedKVCache.fork: sequence {dst!r} exists")
        if src not in self._blocks:
            raise KeyError(f"PagedKVCache.fork: no sequence {src!r}")
        n, bs = self._len[src], self.block_size
        full = n // bs
        if n % bs and not self._free:
            raise RuntimeError("PagedKVCache.fork: the pool is exhausted (1 block needed, 0 free)")
        mine = self._blocks[src][:full]
        for blk in mine:
            self._refs[blk] += 1
        if n % bs:
            old, new = self._blocks[src][full], self._take()
            pools = self.k + self.v + ((self.k_scale + self.v_scale) if self.quantized else [])
            for pool in pools:
                pool[new].copy_(pool[old])
            mine.append(new)
        self._blocks[dst], self._len[dst] = mine, n
        self._root[dst] = self._root[src]
        # what a sequence has in common with its root's keys bounds what any two of a family have in common: a fork of the root shares
        # up to the fork, a fork of a fork no more than its source did
        if self._root[src] == src:
            self._shared[dst] = full * bs
            self._shared[src] = max(self._shared[src], full * bs)
        else:
            self._shared[dst] = min(full * bs, self._shared[src])

    def _pools(self):
        """([k and v pools], [an int8 pool's scale pools]): within a list every pool has one block size in bytes"""
        return self.k + self.v, (self.k_scale + self.v_scale) if self.quantized else []

    def _pool_tables(self):
        """per list of _pools(): (int64 device tensor of base addresses, bytes per block), built once per cache"""
        if self._tables is None:
            self._tables = [(torch.tensor([p.data_ptr() for p in pools], dtype=torch.int64).to(pools[0].device),
                             pools[0][0].numel() * pools[0].element_size()) for pools in self._pools() if pools]
        return self._tables

    def reorder(self, seq_ids: Sequence, parents: Sequence[int]) -> None:
        """Re-point a group of sequences (the beams of a beam search, of any number of prompts; the beams of one prompt have one
        length): afterwards seq_ids[i] holds what seq_ids[parents[i]] held, at its length.  A parent chosen once hands its blocks over, no copy.  A parent chosen m times is shared m ways: its
        first taker gets its blocks, the others share the len // block_size full blocks by reference (one more owner each) and get a fresh
        block with a copy of the partial last block, where there is one -- m - 1 copies.  A sequence nobody chose releases its blocks,
        before the fresh ones are taken.  A seq_ids[i] the cache does not hold yet is admitted by the call (it cannot be a parent).

        Families: the given sequences that had one root are one family afterwards, named by a root object of its own (no sequence id: a
        later fork() of one of them shares no more than it already does), and shared_keys() of each is what ALL of them have in common
        now, the keys of their common leading blocks.  Sequences of the old family outside the call keep their root and are no longer
        in a family with these.

        On GPU pools all copies of the call are one ops.copy_blocks launch (a second one for an int8 pool's scales) over a pointer table
        built once per cache; on CPU pools torch's copy_, as in fork().  Raises, and changes nothing, on bad arguments (ValueError,
        KeyError) or when the pool cannot supply the fresh blocks (RuntimeError)."""
        seq_ids, parents = list(seq_ids), [int(j) for j in parents]
        if len(seq_ids) != len(parents) or not seq_ids or len(set(seq_ids)) != len(seq_ids):
            raise ValueError("PagedKVCache.reorder: seq_ids and parents must be non-empty, of one length, without repeated sequences")
        if any(j < 0 or j >= len(seq_ids) for j in parents):
            raise ValueError(f"PagedKVCache.reorder: every parent must be an index into the {len(seq_ids)} sequences")
        for j in set(parents):
            if seq_ids[j] not in self._blocks:
                raise KeyError(f"PagedKVCache.reorder: no sequence {seq_ids[j]!r}")
        held = [sid in self._blocks for sid in seq_ids]
        bs = self.block_size
        takers: Dict[int, List[int]] = {}
        for i, j in enumerate(parents):
            takers.setdefault(j, []).append(i)
        unchosen = [i for i, h in enumerate(held) if h and i not in takers]
        refs = {}
        for i in unchosen:
            for blk in self._blocks[seq_ids[i]]:
                refs[blk] = refs.get(blk, self._refs[blk]) - 1
        released = sum(1 for r in refs.values() if r == 0)
        fresh = sum(len(t) - 1 for j, t in takers.items() if self._len[seq_ids[j]] % bs)
        if fresh > len(self._free) + released:
            raise RuntimeError(f"PagedKVCache.reorder: the pool is exhausted ({fresh} blocks needed, {len(self._free) + released} free)")
        old = {j: (self._blocks[seq_ids[j]], self._root[seq_ids[j]], self._len[seq_ids[j]]) for j in takers}
        for i in unchosen:
            self.free(seq_ids[i])
        src, dst, groups = [], [], {}
        for j, (blocks, root, n) in old.items():
            full, part = n // bs, n % bs != 0
            for nth, i in enumerate(takers[j]):
                if nth == 0:
                    mine = blocks
                else:
                    mine = blocks[:full]
                    for blk in mine:
                        self._refs[blk] += 1
                    if part:
                        mine.append(self._take())
                        src.append(blocks[full])
                        dst.append(mine[-1])
                self._blocks[seq_ids[i]], self._len[seq_ids[i]] = mine, n
                groups.setdefault(root, []).append(i)
        for members in groups.values():
            lists = [self._blocks[seq_ids[i]] for i in members]
            full, common = min(self._len[seq_ids[i]] for i in members) // bs, 0
            while len(members) > 1 and common < full and all(b[common] == lists[0][common] for b in lists):
                common += 1
            root = _Family()
            for i in members:
                self._root[seq_ids[i]], self._shared[seq_ids[i]] = root, common * bs
        if not src:
            return
        if self.k[0].is_cuda:
            from . import ops

            s, d = (torch.tensor(x, dtype=torch.int32).to(self.k[0].device) for x in (src, dst))
            for table, block_bytes in self._pool_tables():
                ops.copy_blocks(table, s, d, block_bytes, self.num_blocks)
        else:
            for pools in self._pools():
                for pool in pools:
                    pool[dst] = pool[src]

    def root(self, seq_id):
        """The sequence this one's family was forked from (itself, if it never took part in a fork; an object of the family's own once
        reorder() has formed it)."""
        return self._root[seq_id]

    def shared_keys(self, seq_id) -> int:
        """The leading keys, a multiple of block_size, that the sequence has in common with its family (0 without a fork)."""
        return self._shared[seq_id]

    def free(self, seq_id) -> None:
        """Drop a sequence; its blocks go back to the free list (the last one it took is the first to go out again), a shared block only
        with its last owner."""
        if seq_id not in self._blocks:
            raise KeyError(f"PagedKVCache.free: no sequence {seq_id!r}")
        for blk in self._blocks.pop(seq_id):
            self._refs[blk] -= 1
            if self._refs[blk] == 0:
                self._free.append(blk)
        del self._len[seq_id], self._root[seq_id], self._shared[seq_id]

    def length(self, seq_id) -> int:
        return self._len[seq_id]

    def blocks(self, seq_id) -> List[int]:
        return list(self._blocks[seq_id])

    def reserve(self, seq_id, length: int) -> None:
        """Take blocks from the free list until the sequence owns the ceil(length / block_size) blocks that `length` keys need (nothing
        if it owns them already).  The sequence's length does not change: step() takes new blocks only beyond what is owned, and free()
        returns reserved blocks, used or not.  Raises, and changes nothing, when the pool cannot cover it."""
        if seq_id not in self._blocks:
            raise KeyError(f"PagedKVCache.reserve: no sequence {seq_id!r}")
        need = -(-int(length) // self.block_size) - len(self._blocks[seq_id])
        if need > len(self._free):
            raise RuntimeError(f"PagedKVCache.reserve: the pool is exhausted ({need} blocks needed, {len(self._free)} free)")
        for _ in range(need):
            self._blocks[seq_id].append(self._take())

    def advance(self, seq_id, n: int) -> None:
        """Add `n` keys that were written on the device (through the sequence's block table, by a loop the host did not follow token by
        token) to the sequence's length, so that gather() and a later step() see them.  Raises, and changes nothing, if the blocks the
        sequence owns do not hold them: reserve() first."""
        if seq_id not in self._blocks:
            raise KeyError(f"PagedKVCache.advance: no sequence {seq_id!r}")
        n = int(n)
        owned = len(self._blocks[seq_id]) * self.block_size
        if n < 0 or self._len[seq_id] + n > owned:
            raise ValueError(f"PagedKVCache.advance: {self._len[seq_id]} + {n} keys outside the {owned} the sequence's blocks hold")
        self._len[seq_id] += n

    def step(self, seq_ids: Sequence, counts: Sequence[int]) -> PagedStep:
        """Reserve blocks for counts[i] new tokens of sequence seq_ids[i], advance the lengths and return the step's metadata (device
        tensors built on the host, one copy each).  Raises, and changes nothing, when the pool cannot hold the step."""
        seq_ids, counts = list(seq_ids), [int(c) for c in counts]
        if len(seq_ids) != len(counts) or not seq_ids or len(set(seq_ids)) != len(seq_ids):
            raise ValueError("PagedKVCache.step: seq_ids and counts must be non-empty, of one length, without repeated sequences")
        if any(c < 1 for c in counts):
            raise ValueError("PagedKVCache.step: every sequence of a step brings at least one token")
        for sid in seq_ids:
            if sid not in self._blocks:
                raise KeyError(f"PagedKVCache.step: no sequence {sid!r}")
        bs = self.block_size
        need = [-(-(self._len[sid] + c) // bs) - len(self._blocks[sid]) for sid, c in zip(seq_ids, counts)]
        if sum(need) > len(self._free):
            raise RuntimeError(f"PagedKVCache.step: the pool is exhausted ({sum(need)} blocks needed, {len(self._free)} free)")
        starts, pos, slots = [], [], []
        for sid, c, n in zip(seq_ids, counts, need):
            mine = self._blocks[sid]
            for _ in range(n):
                mine.append(self._take())
            start = self._len[sid]
            starts.append(start)
            for p in range(start, start + c):
                pos.append(p)
                slots.append(mine[p // bs] * bs + p % bs)
            self._len[sid] = start + c
        width = max(len(self._blocks[sid]) for sid in seq_ids)
        table = [self._blocks[sid] + [0] * (width - len(self._blocks[sid])) for sid in seq_ids]
        last = [self._len[sid] - 1 for sid in seq_ids]
        dev = self.device
        cu = [0]
        for c in counts:
            cu.append(cu[-1] + c)
        decode = all(c == 1 for c in counts)
        fam = self._families(seq_ids) if decode else None
        family, shared, family_max = fam if fam else (None, None, None)
        return PagedStep(seq_ids=seq_ids, counts=counts, starts=starts, max_len=max(last) + 1, decode=decode,
                         pos=torch.tensor(pos, dtype=torch.int64).to(dev), slots=torch.tensor(slots, dtype=torch.int64).to(dev),
                         block_table=torch.tensor(table, dtype=torch.int32).to(dev), last_pos=torch.tensor(last, dtype=torch.int64).to(dev),
                         cu_tokens=torch.tensor(cu, dtype=torch.int32).to(dev), start_pos=torch.tensor(starts, dtype=torch.int64).to(dev),
                         family=None if family is None else torch.tensor(family, dtype=torch.int32).to(dev),
                         shared=None if shared is None else torch.tensor(shared, dtype=torch.int64).to(dev), family_max=family_max)

    def _families(self, seq_ids):
        """(family, shared, family_max) of a decode step, or None where no two adjacent sequences have one root."""
        family, shared, i, largest = [], [], 0, 1
        while i < len(seq_ids):
            j = i + 1
            while j < len(seq_ids) and self._root[seq_ids[j]] == self._root[seq_ids[i]]:
                j += 1
            common = min(self._shared[sid] for sid in seq_ids[i:j]) if j - i > 1 else 0
            family += [i] * (j - i)
            shared += [common] * (j - i)
            largest = max(largest, j - i)
            i = j
        return (family, shared, largest) if largest > 1 else None

    # ---- reading a sequence back (plain torch; CPU tensors too)

    def gather(self, layer: int, seq_id, length: Optional[int] = None):
        """Contiguous fp16 (k, v) [1, num_kv_heads, length, head_dim] of a sequence's first `length` keys (default: all of them).  An int8
        pool is dequantised as KVCache.dequant does: fp16(float(code) * scale)."""
        n = self._len[seq_id] if length is None else int(length)
        if n < 0 or n > self._len[seq_id]:
            raise ValueError(f"PagedKVCache.gather: length {n} outside the sequence's {self._len[seq_id]} keys")
        nblk = -(-n // self.block_size)
        idx = torch.tensor(self._blocks[seq_id][:nblk], dtype=torch.int64, device=self.k[layer].device)
        out = []
        for pool, scales in ((self.k[layer], self.k_scale[layer] if self.quantized else None),
                             (self.v[layer], self.v_scale[layer] if self.quantized else None)):
            rows = pool.index_select(0, idx).transpose(0, 1).reshape(self.num_kv_heads, nblk * self.block_size, self.head_dim)[:, :n]
            if scales is not None:
                sc = scales.index_select(0, idx).transpose(0, 1).reshape(self.num_kv_heads, nblk * self.block_size)[:, :n]
                rows = (rows.float() * sc[:, :, None]).half()
            out.append(rows[None].contiguous())
        return tuple(out)


__all__ = ["PagedKVCache", "PagedStep"]
