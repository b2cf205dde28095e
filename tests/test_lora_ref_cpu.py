"""Multi-LoRA without a GPU: the f64 reference and its derived bound on every GPU case's inputs, what the header declares,
the entry's argument checks (before any launch), the op's own refusals and fake registration, LoraBank's loader and generate()'s
`adapters` check."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lora_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qqq_amd_lora.h")
ERR_ARG = 17


# ---- the reference

@pytest.fixture(scope="module")
def computed():
    out = []
    for c in lora_ref.CASES:
        d = lora_ref.inputs(c)
        out.append((c, d, lora_ref.reference(d["y"][:, :d["N"]], d["xq"], d["s1"], d["A"], d["B"], d["scale"], d["slot"], d["part_cols"])))
    return out


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    cs = lora_ref.CASES
    assert {c[1] for c in cs} == {128, 192, 11008} and {c[3] for c in cs} == {8, 16, 64} and {c[0] for c in cs} == {1, 2, 15, 16, 17, 70}
    assert {c[2] for c in cs if len(c[4]) == 2} == {128, 320}
    assert (0, 128, 256) in {c[4] for c in cs} and (0, 256, 320, 384) in {c[4] for c in cs} and any(c[6] > c[2] for c in cs)
    assert {c[5] for c in cs} == {"none", "same", "distinct16", "runs", "last", "interleaved"}
    assert [c for c in cs if c[1] == 11008] == [(2, 11008, 128, 16, (0, 128), "last", 128)]
    s = lora_ref.slots_of("distinct16", 16)
    assert len(set(s.tolist())) == 16 and s.min() >= 0 and s.max() < lora_ref.S
    runs = lora_ref.slots_of("runs", 70)
    assert runs[15] == runs[16] and runs[31] == runs[32] and runs[17] != runs[18]  # runs across the 16-token tile boundaries
    assert lora_ref.slots_of("last", 17).max() == lora_ref.S - 1 and (lora_ref.slots_of("interleaved", 70) == -1).sum() == 24


def test_the_reference_is_finite_and_the_bound_is_tight(computed):
    tight = total = 0
    for c, d, (val, bound, touched) in computed:
        assert np.isfinite(val).all() and np.isfinite(bound).all() and (bound >= 0).all(), lora_ref.case_id(c)
        y0 = d["y"][:, :d["N"]].astype(np.float64)
        assert np.array_equal(val[~touched], y0[~touched]) and not bound[~touched].any()
        assert np.array_equal(touched, d["slot"] >= 0)
        if touched.any():
            assert np.abs(val[touched] - y0[touched]).mean() > 8 * lora_ref.fp16_ulp(val[touched]).mean() / 4  # the adapters are visible
            tight += int((bound[touched] < lora_ref.fp16_ulp(val[touched])).sum())
            total += bound[touched].size
    print(f"bound below one fp16 ulp on {tight} of {total} elements ({tight / total:.4f})")
    assert tight >= 0.99 * total


def test_check_takes_the_rounded_reference_and_refuses_an_ulp(computed):
    c, d, (val, bound, touched) = computed[3]
    rounded = val.astype(np.float16)
    assert lora_ref.check(rounded, val, bound).all()
    off = (rounded.view(np.uint16) + 2).view(np.float16)  # two ulps away
    tight = touched[:, None] & (bound < 0.25 * lora_ref.fp16_ulp(val))  # (the few values next to zero have a bound of several of their ulps)
    assert tight.mean() > 0.9 and not lora_ref.check(off, val, bound)[tight].any()
    assert np.array_equal(lora_ref.fp16_ulp(np.array([1.0, 1.5, 2.0, 0.75, 1e-9, -3.0])), [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -9])


def test_padding_an_adapter_to_a_larger_rank_changes_nothing(computed):
    c, d, (val, bound, _) = computed[7]  # two parts
    R, P = d["B"].shape[2], len(d["part_cols"]) - 1
    A2 = np.zeros((lora_ref.S, P * 2 * R, d["A"].shape[2]), np.float16)
    for p in range(P):
        A2[:, p * 2 * R:p * 2 * R + R] = d["A"][:, p * R:(p + 1) * R]
    B2 = np.concatenate([d["B"], np.zeros_like(d["B"])], axis=2)
    val2, _, _ = lora_ref.reference(d["y"][:, :d["N"]], d["xq"], d["s1"], A2, B2, d["scale"], d["slot"], d["part_cols"])
    assert np.array_equal(val2, val)


# ---- the header, the binding, the entry's checks

@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def test_the_header_declares_the_entry(L):
    from qqq_amd import _abi, _lib, build

    assert _lib.ABI_VERSION == 4 and L.qqq_amd_abi_version() == 4
    protos = _abi.prototypes(HEADER)
    assert set(protos) == {"qqq_lora_add"} and len(protos["qqq_lora_add"][1]) == 19
    assert L.qqq_lora_add.restype is ctypes.c_int and len(L.qqq_lora_add.argtypes) == 19
    unit = open(build.SRC).read()
    assert '#include "qqq_lora.hip.h"' in unit and '#include "../../include/qqq_amd_lora.h"' in unit


A16, A4, A2 = 0x20010, 0x30004, 0x40002  # fake device addresses: every call below must fail in the checks, before any launch


def _call(L, cols=(0, 128), y=A4, ldy=128, xq=A16, s1=A4, A=A16, a_stride=16 * 128, B=A16, b_stride=128 * 16, scale=A4, slot=A4, P=1, T=4,
          N=128, K=128, R=16, S=2):
    arr = (ctypes.c_int * len(cols))(*cols) if cols is not None else None
    return L.qqq_lora_add(y, ldy, xq, s1, A, a_stride, B, b_stride, scale, slot, arr, P, T, N, K, R, S, 0, None)


def test_argument_errors_come_back_as_messages(L):
    from qqq_amd import _lib

    def refused(text, **kw):
        assert _call(L, **kw) == ERR_ARG
        assert _lib.last_error().startswith("qqq_lora_add: ") and text in _lib.last_error(), _lib.last_error()

    assert _call(L, T=0, y=0, xq=0, cols=None) == 0  # a no-op, NULL pointers allowed
    refused("T=-1 outside", T=-1)
    for r in (0, 4, 12, 24, 128):
        refused(f"R={r} is not one of 8, 16, 32, 64", R=r)
    refused("bad shape N=100", N=100, cols=(0, 100), ldy=100)
    refused("bad shape N=128 K=96", K=96)
    refused("bad shape", S=0)
    refused("bad shape", P=4, cols=(0, 64, 128, 192, 256), N=256, ldy=256)
    refused("ldy=126", ldy=126)
    refused("ldy=129", ldy=129)
    refused("part_cols must be non-NULL", cols=None)
    for cols, P in (((0, 64), 1), ((64, 128), 1), ((0, 96, 128), 2), ((0, 128, 128), 2), ((0, 128, 64, 128), 3), ((0, 64, 192), 2)):
        refused("part_cols must ascend strictly from 0 to N=128 in multiples of 64", cols=cols, P=P, a_stride=P * 16 * 128)
    refused("bad slot stride", a_stride=16 * 128 - 8)
    refused("bad slot stride", a_stride=16 * 128 + 4)
    refused("bad slot stride", b_stride=128 * 16 - 8)
    for name, bad in (("y", A2), ("xq", A4), ("s1", A2), ("A", A4), ("B", A4), ("scale", A2), ("slot", A2), ("y", 0), ("slot", 0)):
        refused("bad argument (every pointer must be non-NULL; xq, A and B 16-byte, everything else 4-byte aligned)", **{name: bad})


def test_the_ops_own_refusals_and_its_fake_registration():
    from qqq_amd import ops

    t = dict(y=torch.zeros((4, 128), dtype=torch.float16), xq=torch.zeros((4, 128), dtype=torch.int8), s1=torch.ones((4, 1)),
             A=torch.zeros((2, 32, 128), dtype=torch.float16), B=torch.zeros((2, 128, 16), dtype=torch.float16), scale=torch.ones(2),
             slot=torch.zeros(4, dtype=torch.int32))
    order = ("y", "xq", "s1", "A", "B", "scale", "slot")
    check = lambda cols=(0, 64, 128), **kw: ops._lora_add_check(*[kw.get(k, t[k]) for k in order], cols)  # noqa: E731
    assert check() == (4, 128, 128, 16, 2, 2)
    assert check(A=torch.zeros((2, 16, 128), dtype=torch.float16), cols=(0, 128)) == (4, 128, 128, 16, 2, 1)
    assert check(A=torch.zeros((5, 64, 128), dtype=torch.float16)[:2, 16:48]) == (4, 128, 128, 16, 2, 2)  # a view with its own slot stride
    assert check(y=torch.zeros((4, 256), dtype=torch.float16)[:, 64:192]) == (4, 128, 128, 16, 2, 2)     # a column slice of a fused output
    for name, bad in (("y", t["y"].float()), ("xq", t["xq"].int()), ("s1", t["s1"].half()), ("A", t["A"].float()), ("B", t["B"].bfloat16()),
                      ("scale", t["scale"].double()), ("slot", t["slot"].long())):
        with pytest.raises(RuntimeError, match=f"lora_add: {name} must be "):
            check(**{name: bad})
    with pytest.raises(RuntimeError, match="lora_add: with y"):
        check(cols=(0, 128))
    with pytest.raises(RuntimeError, match="lora_add: s1 must be f32 \\[4\\] or \\[4, 1\\] and slot int32 \\[4\\]"):
        check(slot=t["slot"][:3])
    with pytest.raises(RuntimeError, match="lora_add: y must have unit column stride"):
        check(y=torch.zeros((128, 4), dtype=torch.float16).t())
    with pytest.raises(RuntimeError, match="lora_add: A and B must have contiguous rows and columns"):
        check(B=torch.zeros((2, 16, 128), dtype=torch.float16).transpose(1, 2))
    with pytest.raises(RuntimeError, match="lora_add: every tensor must be on the GPU"):
        ops.lora_add(*[t[k] for k in order], (0, 64, 128))
    assert ops._lora_add_op._opoverload.name() == "qqq_amd::lora_add"
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode() as mode:
        fake = [mode.from_tensor(t[k]) for k in order]
        assert torch.ops.qqq_amd.lora_add(*fake, [0, 64, 128]) is None
        with pytest.raises(RuntimeError, match="lora_add: with y"):
            torch.ops.qqq_amd.lora_add(*fake, [0, 128])


# ---- the loader and the keyword

def test_peft_names_are_matched():
    from qqq_amd.lora import parse_key

    assert parse_key("base_model.model.model.layers.11.self_attn.q_proj.lora_A.weight") == (11, "q_proj", "A")
    assert parse_key("layers.0.mlp.down_proj.lora_B.default.weight") == (0, "down_proj", "B")
    assert parse_key("model.layers.3.mlp.gate_proj.lora_A.default.weight") == (3, "gate_proj", "A")
    for bad in ("layers.0.mlp.q_proj.lora_A.weight", "layers.0.self_attn.down_proj.lora_B.weight", "layers.0.self_attn.q_proj.weight",
                "layers.0.self_attn.q_proj.lora_C.weight", "layers.x.self_attn.q_proj.lora_A.weight", "mylayers.0.self_attn.q_proj.lora_A.weight",
                "layers.0.self_attn.q_proj.lora_A.other.weight", "layers.0.self_attn.q_proj.lora_A.weight.extra", "lm_head.lora_A.weight"):
        assert parse_key(bad) is None, bad


@pytest.fixture(scope="module")
def tiny():
    from qqq_amd import QuantLlamaForCausalLM, QuantLlamaModel

    return QuantLlamaForCausalLM(QuantLlamaModel(64, 2, 128, 2, 1, 256, -1))


def _sd(r=8, layers=(0, 1), projs=(("self_attn", "q_proj", 128, 128), ("self_attn", "v_proj", 128, 64), ("mlp", "down_proj", 256, 128))):
    g = torch.Generator().manual_seed(1)
    sd = {}
    for li in layers:
        for parent, name, k, n in projs:
            sd[f"model.layers.{li}.{parent}.{name}.lora_A.weight"] = torch.randn((r, k), generator=g)
            sd[f"model.layers.{li}.{parent}.{name}.lora_B.default.weight"] = torch.randn((n, r), generator=g)
    return sd


def test_the_bank_stores_every_group_once_and_loads_in_place(tiny):
    from qqq_amd import LoraBank

    bank = LoraBank(tiny, slots=3, rank=16)
    g = bank.groups[1]
    assert set(g) == {"q_proj", "k_proj", "v_proj", "qkv", "o_proj", "gate_proj", "up_proj", "gate_up", "down_proj"}
    A, B, scale, cols = g["qkv"]
    assert A.shape == (3, 48, 128) and B.shape == (3, 256, 16) and cols == (0, 128, 192, 256) and scale is bank.scale
    assert g["gate_up"][0].shape == (3, 32, 128) and g["gate_up"][3] == (0, 256, 512) and g["down_proj"][0].shape == (3, 16, 256)
    vA, vB, _, vcols = g["v_proj"]  # the single projections are views of the group's storage
    assert vA.data_ptr() == A[0, 32].data_ptr() and vA.stride() == A.stride() and vB.data_ptr() == B[0, 192].data_ptr() and vcols == (0, 64)
    assert bank.nbytes == sum(t.numel() * 2 for t in bank._storage) + 12 and len(bank._storage) == 2 * 4 * 2
    sd = _sd()
    bank.load(1, sd, alpha=32)
    assert float(bank.scale[1]) == 4.0 and float(bank.scale[0]) == 0.0
    assert torch.equal(vA[1, :8], sd["model.layers.1.self_attn.v_proj.lora_A.weight"].half()) and not vA[1, 8:].any() and not vA[0].any()
    assert torch.equal(vB[1, :, :8], sd["model.layers.1.self_attn.v_proj.lora_B.default.weight"].half()) and not vB[1, :, 8:].any()
    assert not g["k_proj"][0].any() and not g["gate_up"][1].any()  # projections the adapter lacks stay zero
    addresses = [t.data_ptr() for t in bank._storage]
    bank.load(1, _sd(r=16, layers=(0,)), alpha=8)  # a second load replaces the first
    assert float(bank.scale[1]) == 0.5 and not vA[1].any() and bank.groups[0]["v_proj"][0][1].any()
    bank.unload(1)
    assert not any(t.any() for t in bank._storage) and not bank.scale.any() and addresses == [t.data_ptr() for t in bank._storage]
    part = LoraBank(tiny, slots=1, rank=8, targets=("q_proj", "v_proj", "up_proj"))
    assert set(part.groups[0]) == {"q_proj", "v_proj", "up_proj"} and part.groups[0]["v_proj"][0].data_ptr() == part._storage[0][0, 8].data_ptr()
    step = part.step(part.token_slots([0, -1, 0]))
    assert step.layer(0)("qkv") is None and step.layer(0)("k_proj") is None and step.layer(0)("v_proj")[3] is step.token_slot


def test_a_load_that_fails_leaves_the_slot_untouched(tiny):
    from qqq_amd import LoraBank

    bank = LoraBank(tiny, slots=2, rank=8)
    bank.load(0, _sd(), alpha=16)
    before = [t.clone() for t in bank._storage] + [bank.scale.clone()]
    good = _sd()
    key = "model.layers.0.self_attn.q_proj.lora_A.weight"
    cases = [
        (dict(good, **{"model.layers.0.self_attn.q_proj.weight": torch.zeros(1, 1)}), "unknown key"),
        (dict(good, **{"model.layers.2.self_attn.q_proj.lora_A.weight": torch.zeros(8, 128)}), "names a projection the bank does not hold"),
        (_sd(r=16), "has rank 16, the bank holds ranks 1 ... 8"),
        (dict(good, **{key: torch.zeros(8, 64)}), "needs lora_A \\[8, 128\\] and lora_B \\[128, 8\\]"),
        (dict(good, **{key: torch.zeros(4, 128)}), "needs lora_A \\[4, 128\\] and lora_B \\[128, 4\\]"),
        ({k: v for k, v in good.items() if k != "model.layers.1.mlp.down_proj.lora_B.default.weight"}, "layers.1.down_proj has lora_A without lora_B"),
        ({k: v for k, v in good.items() if k != key}, "layers.0.q_proj has lora_B without lora_A"),
        (dict(good, **{"x.layers.0.self_attn.q_proj.lora_A.default.weight": torch.zeros(8, 128)}), "is given twice"),
        ({}, "holds no adapter matrices"),
    ]
    for sd, text in cases:
        with pytest.raises(ValueError, match="LoraBank.load: .*" + text):
            bank.load(0, sd, alpha=16)
        assert all(torch.equal(a, b) for a, b in zip([*bank._storage, bank.scale], before)), text
    for bad in (-1, 2, True, 1.0):
        with pytest.raises(ValueError, match="outside \\[0, 2\\)"):
            bank.load(bad, good, alpha=16)
        with pytest.raises(ValueError, match="outside \\[0, 2\\)"):
            bank.unload(bad)
    with pytest.raises(ValueError, match="slot 2 outside \\[-1, 2\\)"):
        bank.token_slots([0, 2])
    for kw, text in ((dict(slots=0, rank=8), "slots=0"), (dict(slots=1, rank=12), "rank=12 is not one of"), (dict(slots=1, rank=8, targets=("x",)), "targets")):
        with pytest.raises(ValueError, match="LoraBank: .*" + text):
            LoraBank(tiny, **kw)


def test_generate_checks_adapters_with_the_other_keywords(tiny):
    from qqq_amd import LoraBank
    from qqq_amd.request import Request, adapter_slots

    bank = LoraBank(tiny, slots=3, rank=8)
    assert adapter_slots("generate", bank, [0, None, 2], 3) == [0, -1, 2] and adapter_slots("generate", None, None, 2) == [-1, -1]
    for bad, text in (([0, 1], "one entry per prompt \\(3\\)"), (7, "one entry per prompt"), ("012", "one entry per prompt"),
                      ([0, 3, 1], "neither None nor a slot in \\[0, 3\\)"), ([0, -1, 1], "neither None"), ([0, True, 1], "neither None"),
                      ([0, 1.5, 1], "neither None")):
        with pytest.raises(ValueError, match="generate: adapters .*" + text):
            adapter_slots("generate", bank, bad, 3)
    args = ("generate", 64, 0.0, 0, 1.0, None, None, 1.0, 0.0, 0.0, None, None, 0, 1, None)
    with pytest.raises(ValueError, match="generate: adapters need lora"):
        Request(*args, adapters=[0])
    with pytest.raises(ValueError, match="generate: lora must be a LoraBank"):
        Request(*args, lora=object())
    req = Request(*args, lora=bank, adapters=[1, None])
    req.begin([[1, 2], [3]])
    assert req.slots == [1, -1] and req.loop_keywords() == ({"lora": bank}, {"adapters": [1, None]})
    assert Request(*args).loop_keywords() == ({}, {})
    with pytest.raises(ValueError, match="generate: adapters need lora"):
        tiny.generate([[1, 2]], 2, adapters=[0])
