"""Multi-LoRA serving over the quantised base: the int4 weights are shared, every tenant brings fp16 low-rank matrices, and the adapters of
one batch are mixed per token by ops.lora_add (include/qqq_amd_lora.h) on the output of every targeted projection.

    LoraBank   the stacked adapters of a model: `slots` adapter slots of rank `rank`, per layer the A / B of four projection groups
               (q|k|v, o, gate|up, down) at addresses that stay fixed for the bank's life, so a captured graph survives load() / unload()
    LoraStep   what PagedStep.lora holds: the bank and the step's token_slot (int32 [tokens] on the device, -1: no adapter)

A group's tensors are stored once: A [slots, P * rank, K] and B [slots, N, rank] over the P targeted projections of the group, which
share their input.  When all of a group is targeted the fused holders (fuse_qkv(), fuse_gate_up()) serve it with one launch; the single
projections take views of the same storage (their rows of A, their columns' rows of B), with the group's slot stride.
"""
from __future__ import annotations

import re
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
RANKS = (8, 16, 32, 64)
_GROUPS = (("self_attn", "qkv", ("q_proj", "k_proj", "v_proj")), ("self_attn", "o", ("o_proj",)),
           ("mlp", "gate_up", ("gate_proj", "up_proj")), ("mlp", "down", ("down_proj",)))
_PARENT = {proj: parent for parent, _, members in _GROUPS for proj in members}
_KEY = re.compile(r"(?:^|.*\.)layers\.(\d+)\.(self_attn|mlp)\.(\w+)\.lora_([AB])(?:\.default)?\.weight$")


def parse_key(key: str) -> Optional[Tuple[int, str, str]]:
    """a PEFT-style name -> (layer, projection, "A" or "B"); None if it is not one (any prefix; `.lora_A.weight` or `.lora_A.default.weight`)"""
    m = _KEY.match(key)
    if not m or _PARENT.get(m.group(3)) != m.group(2):
        return None
    return int(m.group(1)), m.group(3), m.group(4)


class LayerLora:
    """One layer's view of a LoraStep: layer_lora(name) -> the (A, B, scale, slot, part_cols) that QuantLinear.forward_int8(lora=) takes for the
    projection or fused group `name` ("q_proj" ... "down_proj", "qkv", "gate_up"), None where the bank holds nothing for it."""
    __slots__ = ("groups", "slot")

    def __init__(self, groups: Dict[str, tuple], slot: torch.Tensor):
        self.groups, self.slot = groups, slot

    def __call__(self, name: str):
        g = self.groups.get(name)
        return None if g is None else (g[0], g[1], g[2], self.slot, g[3])


class LoraStep(NamedTuple):
    """PagedStep.lora: the bank and the adapter slot of every token of the step (int32 [tokens] on the bank's device, -1: none)"""
    bank: "LoraBank"
    token_slot: torch.Tensor

    def layer(self, index: int) -> LayerLora:
        return LayerLora(self.bank.groups[index], self.token_slot)


class LoraBank:
    """LoraBank(lm, slots, rank, targets): storage for `slots` adapters of rank <= `rank` on the projections `targets` of every decoder layer
    of `lm` (a QuantLlamaForCausalLM), on its device, zeroed: an empty slot adds nothing.  load() / unload() rewrite a slot in place.

    groups[layer][name] = (A, B, scale, part_cols) for every targeted projection, and for "qkv" / "gate_up" when all of the group is
    targeted.  A projection outside `targets` has no tensors and runs no op."""

    def __init__(self, lm, slots: int, rank: int, targets: Sequence[str] = TARGETS):
        slots, rank, targets = int(slots), int(rank), tuple(targets)
        if slots < 1:
            raise ValueError(f"LoraBank: slots={slots} must be at least 1")
        if rank not in RANKS:
            raise ValueError(f"LoraBank: rank={rank} is not one of {RANKS}")
        unknown = [t for t in targets if t not in TARGETS]
        if unknown or not targets:
            raise ValueError(f"LoraBank: targets must be a non-empty subset of {TARGETS}, not {targets}")
        self.slots, self.rank, self.targets = slots, rank, tuple(t for t in TARGETS if t in targets)
        dev = lm.lm_head.weight.device
        self.device = dev
        self.scale = torch.zeros(slots, dtype=torch.float32, device=dev)
        self.groups = []   # per layer: name -> (A, B, scale, part_cols)
        self._where = []   # per layer: projection -> (group A, group B, first row of A, first row of B, N, K)
        self._storage = []
        for layer in lm.model.layers:
            groups, where = {}, {}
            for parent, fused, members in _GROUPS:
                held = [m for m in members if m in self.targets]
                if not held:
                    continue
                mods = [getattr(getattr(layer, parent), m) for m in held]
                K, widths = mods[0].infeatures, [m.outfeatures for m in mods]
                A = torch.zeros((slots, len(held) * rank, K), dtype=torch.float16, device=dev)
                B = torch.zeros((slots, sum(widths), rank), dtype=torch.float16, device=dev)
                self._storage += [A, B]
                cols = [0]
                for j, (name, n) in enumerate(zip(held, widths)):
                    groups[name] = (A[:, j * rank:(j + 1) * rank], B[:, cols[-1]:cols[-1] + n], self.scale, (0, n))
                    where[name] = (A, B, j * rank, cols[-1], n, K)
                    cols.append(cols[-1] + n)
                if len(held) == len(members) > 1:
                    groups[fused] = (A, B, self.scale, tuple(cols))
            self.groups.append(groups)
            self._where.append(where)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self._storage) + self.scale.numel() * 4

    def _slot(self, what: str, slot) -> int:
        if isinstance(slot, bool) or not isinstance(slot, int) or not 0 <= slot < self.slots:
            raise ValueError(f"LoraBank.{what}: slot={slot!r} outside [0, {self.slots})")
        return slot

    def step(self, token_slot: torch.Tensor) -> LoraStep:
        return LoraStep(self, token_slot)

    def token_slots(self, slots: Sequence[int]) -> torch.Tensor:
        """host slots (one per token, -1: none), checked against the bank -> the int32 device tensor a LoraStep takes"""
        slots = [int(s) for s in slots]
        bad = [s for s in slots if not -1 <= s < self.slots]
        if bad:
            raise ValueError(f"LoraBank: slot {bad[0]} outside [-1, {self.slots})")
        return torch.tensor(slots, dtype=torch.int32).to(self.device)

    @torch.no_grad()
    def load(self, slot: int, state_dict: Dict[str, torch.Tensor], alpha: float) -> None:
        """Write an adapter into `slot`: PEFT-style names (parse_key), lora_A.weight [r, K] and lora_B.weight [N, r] per projection, cast to
        fp16, zero-padded from r to the bank's rank; projections the adapter lacks stay zero; the slot's scale becomes alpha / r.  Raises
        on the first problem -- an unknown key, a projection outside the bank, a shape mismatch, a rank above the bank's, ranks that
        differ, A without B -- and leaves the slot as it was."""
        slot = self._slot("load", slot)
        found: Dict[Tuple[int, str], Dict[str, torch.Tensor]] = {}
        for key, t in state_dict.items():
            at = parse_key(key)
            if at is None:
                raise ValueError(f"LoraBank.load: unknown key {key!r} (expected ...layers.N.self_attn|mlp.PROJ.lora_A|lora_B[.default].weight)")
            li, proj, which = at
            if li >= len(self._where) or proj not in self._where[li]:
                raise ValueError(f"LoraBank.load: {key!r} names a projection the bank does not hold ({len(self._where)} layers, targets {self.targets})")
            if not isinstance(t, torch.Tensor) or t.dim() != 2:
                raise ValueError(f"LoraBank.load: {key!r} must be a two-dimensional tensor")
            if which in found.setdefault((li, proj), {}):
                raise ValueError(f"LoraBank.load: {key!r} is given twice")
            found[(li, proj)][which] = t
        if not found:
            raise ValueError("LoraBank.load: the state-dict holds no adapter matrices")
        r = None
        for (li, proj), ab in found.items():
            if set(ab) != {"A", "B"}:
                raise ValueError(f"LoraBank.load: layers.{li}.{proj} has lora_{min(ab)} without lora_{'B' if 'A' in ab else 'A'}")
            _, _, _, _, n, k = self._where[li][proj]
            ra = ab["A"].shape[0]
            if ra < 1 or ra > self.rank:
                raise ValueError(f"LoraBank.load: layers.{li}.{proj} has rank {ra}, the bank holds ranks 1 ... {self.rank}")
            if tuple(ab["A"].shape) != (ra, k) or tuple(ab["B"].shape) != (n, ra):
                raise ValueError(f"LoraBank.load: layers.{li}.{proj} needs lora_A [{ra}, {k}] and lora_B [{n}, {ra}], not "
                                 f"{tuple(ab['A'].shape)} and {tuple(ab['B'].shape)}")
            if r is not None and ra != r:
                raise ValueError(f"LoraBank.load: layers.{li}.{proj} has rank {ra}, other projections of the adapter {r}")
            r = ra
        self.unload(slot)
        for (li, proj), ab in found.items():
            A, B, a0, b0, n, _ = self._where[li][proj]
            A[slot, a0:a0 + r] = ab["A"].to(device=self.device, dtype=torch.float16)
            B[slot, b0:b0 + n, :r] = ab["B"].to(device=self.device, dtype=torch.float16)
        self.scale[slot] = float(alpha) / r

    @torch.no_grad()
    def unload(self, slot: int) -> None:
        """zero the slot: its rows then add nothing"""
        slot = self._slot("unload", slot)
        for t in self._storage:
            t[slot].zero_()
        self.scale[slot] = 0.0


__all__ = ["LoraBank", "LoraStep", "LayerLora", "parse_key", "TARGETS", "RANKS"]
