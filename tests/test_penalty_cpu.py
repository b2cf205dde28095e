"""The repetition / presence / frequency penalty without a GPU: tests/penalty_ref.py against rows computed by hand, the C-ABI of
include/qqq_amd_penalty.h (declared set, exports, the workspace size, argument checks before any launch, the NULL no-op), the kernel's
resources in the gfx950 code object, the op's refusals and fake implementation, and the bookkeeping of the two loops and of
QuantLlamaForCausalLM.generate over host stubs of the forward pass and the ops."""
import os
import sys

import numpy as np
import pytest
import torch

import penalty_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 17
f16, f32 = np.float16, np.float32


# ---- the restatement against rows computed by hand

def test_rule_by_hand():
    # 3 / 1.5 = 2;  -3 * 1.5 = -4.5;  a zero is "not > 0": 0 * 1.5 = 0, -0 * 1.5 = -0
    assert penalty_ref.rule(f16(3), 0, 1.5, 9, 9) == f16(2) and penalty_ref.rule(f16(-3), 0, 1.5, 9, 9) == f16(-4.5)
    assert penalty_ref.rule(f16(-0.0), 0, 1.5, 0, 0).view(np.uint16) == 0x8000 and penalty_ref.rule(f16(0.0), 0, 1.5, 0, 0).view(np.uint16) == 0
    # c = 3 outputs: 2 - 0.25 * 3 - 0.5 = 0.75, and after the repetition rule: 4 / 2 - 0.75 - 0.5 = 0.75
    assert penalty_ref.rule(f16(2), 3, 1, 0.5, 0.25) == f16(0.75) and penalty_ref.rule(f16(4), 3, 2, 0.5, 0.25) == f16(0.75)
    # two roundings, not one: fl(0.1f * 3) = 0.3000000119..., 1 - that = 0.699999988 -> fp16 0.7002 (0x399a)
    assert penalty_ref.rule(f16(1), 3, 1, 0, f32(0.1)).view(np.uint16) == f16(f32(1) - f32(f32(0.1) * f32(3))).view(np.uint16)
    # overflow of fp16 and the specials, carried out as written
    assert penalty_ref.rule(f16(-60000), 1, 1, 10000, 0) == f16(-np.inf) and penalty_ref.rule(f16(np.inf), 2, 2, 1, 1) == f16(np.inf)
    assert np.isnan(penalty_ref.rule(f16(np.nan), 2, 2, 1, 1)) and penalty_ref.rule(f16(-np.inf), 0, 2, 0, 0) == f16(-np.inf)
    assert penalty_ref.rule(f16(60000), 0, 0.5, 0, 0) == f16(np.inf)  # 120000 is past fp16


def test_rows_by_hand():
    vocab, ld = 7, 8
    base = np.array([1, -1, 2, -2, 4, -4, 0.5, 99], dtype=f16)
    logits = np.tile(base, (6, 1))  # rows 0 .. 2 of G = 2 logits rows each
    ids = np.array([[3, 5], [6, 6], [1, 1]], dtype=np.int64)
    pos = np.array([[2, 3], [-1, 0], [1, 2]], dtype=np.int64)
    seen = np.array([[0, 3, 9, 9], [1, 2, 3, 4], [7, 0, 0, 0]], dtype=np.int32)  # row 0: prompt [0], outputs [3, 3]; row 2 holds an invalid 7
    got, seen2 = penalty_ref.penalize(logits, ids, pos, seen, np.array([1, 0, 0], np.int32), 2.0, 0.5, 0.25, vocab)
    exp = logits.copy()
    # row 0, j = 0: S = [0 | 3, 3]: token 0 (prompt only) 1 / 2; token 3 (c = 2): -2 * 2 - 0.5 - 0.5
    exp[0, 0], exp[0, 3] = 0.5, -5.0
    # row 0, j = 1: the draft 5 at index 3, an output: -4 * 2 - 0.25 - 0.5
    exp[1, 0], exp[1, 3], exp[1, 5] = 0.5, -5.0, -8.75
    # row 1 idle: nothing.  row 2: seen[2, 1] = 1 is recorded; the 7 counts for nothing; j = 0: token 1, c = 1; j = 1: c = 2
    exp[4, 1], exp[5, 1] = -2.75, -3.0
    assert np.array_equal(got.view(np.uint16), exp.view(np.uint16))
    assert seen2.tolist() == [[0, 3, 3, 9], [1, 2, 3, 4], [7, 1, 0, 0]] and seen[0, 2] == 9 and logits[0, 0] == 1  # the inputs are left alone
    # a neutral row is recorded but keeps its logits; n_prompt past the drafts leaves the repetition rule alone
    got, seen2 = penalty_ref.penalize(logits, ids, pos, seen, np.array([9, 9, 9], np.int32), np.array([1, 2, 2], f32),
                                      np.array([0, 5, 5], f32), np.array([0, 5, 5], f32), vocab)
    exp = logits.copy()
    exp[4, 1], exp[5, 1] = -2, -2
    assert np.array_equal(got.view(np.uint16), exp.view(np.uint16)) and seen2[0].tolist() == [0, 3, 3, 9]
    # ids outside [0, vocab) are recorded as -1 and count for nothing
    got, seen2 = penalty_ref.penalize(logits[:2], np.array([[7, -1]]), np.array([[0, 1]]), seen[:1], np.array([0], np.int32), 2.0, 1, 1, vocab)
    assert np.array_equal(got.view(np.uint16), logits[:2].view(np.uint16)) and seen2[0].tolist() == [-1, 3, 9, 9]


# ---- the C-ABI

@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def test_header_declares_the_entries_and_the_library_exports_them(L):
    from qqq_amd import _abi

    names = set(_abi.prototypes(os.path.join(ROOT, "include", "qqq_amd_penalty.h")))
    assert names == {"qqq_penalize_logits", "qqq_penalize_logits_workspace_bytes"}
    for n in names:
        assert hasattr(L, n), n
    assert L.qqq_amd_abi_version() == 4
    main = _abi.source(os.path.join(ROOT, "include", "qqq_amd.h"))
    assert "qqq_penal" not in main  # the feature has its own header (a newer one rebuilds the library: tests/test_abi_cpu.py)


def test_workspace_bytes(L):
    assert L.qqq_penalize_logits_workspace_bytes(6, 1003) == 6 * 1003 * 4
    assert L.qqq_penalize_logits_workspace_bytes(65535, 262144) == 65535 * 262144 * 4  # past 2^32: a size_t
    for rows, vocab in ((0, 1003), (-1, 1003), (65536, 8), (6, 0), (6, -5), (6, 262145)):
        assert L.qqq_penalize_logits_workspace_bytes(rows, vocab) == 0, (rows, vocab)


# fake device addresses with the alignment the entry point asks for: the calls below must fail in the checks, before any launch
A8, A4, A2 = 0x20008, 0x30004, 0x40002
PTRS = dict(logits=A2, ids=A8, pos=A8, seen=A4, n_prompt=A4, rep=A4, pres=A4, freq=A4, ws=A4)


def _call(L, ld=1003, group=3, seen_stride=64, ws_bytes=6 * 1003 * 4, rows=6, vocab=1003, **ptrs):
    a = dict(PTRS, **ptrs)
    return L.qqq_penalize_logits(a["logits"], ld, a["ids"], a["pos"], group, a["seen"], seen_stride, a["n_prompt"], a["rep"], a["pres"],
                                 a["freq"], a["ws"], ws_bytes, rows, vocab, 0, None)


BAD = ([{name: None} for name in PTRS] + [dict(logits=A2 + 1)] + [{name: A8 + 4} for name in ("ids", "pos")]
       + [{name: A4 + 2} for name in ("seen", "n_prompt", "rep", "pres", "freq", "ws")]
       + [dict(group=0), dict(group=-1), dict(group=17), dict(seen_stride=0), dict(seen_stride=-4), dict(seen_stride=1 << 30)]
       + [dict(ws_bytes=6 * 1003 * 4 - 1), dict(ws_bytes=0), dict(ld=1002), dict(ld=0), dict(vocab=0, ld=8), dict(vocab=262145, ld=262152),
          dict(rows=-1), dict(rows=65536, group=1), dict(rows=21846, group=3), dict(rows=4096, group=16)])


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_penalize_logits_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _call(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_penalize_logits:")


def test_rows_0_is_a_no_op_with_null_pointers(L):
    z = None
    assert L.qqq_penalize_logits(z, 0, z, z, 0, z, 0, z, z, z, z, z, 0, 0, 0, 0, z) == 0
    assert _call(L, rows=0) == 0


def test_penalty_kernel_in_the_code_object_without_scratch_or_spills():
    """One kernel, sixteen waves, no scratch, a few registers and the 64 bytes of LDS that hold the drafts."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB)}
    assert {n for n in ks if "penal" in n} == {"qqq_penalize_logits_kernel"}
    k = ks["qqq_penalize_logits_kernel"]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["max_flat_workgroup_size"] == 1024 and k["vgpr_count"] + k["agpr_count"] <= 64 and k["group_segment_fixed_size"] <= 64, k


# ---- the op without a GPU

def _op_args(rows=3, g=2, vocab=40, stride=9, device="cpu"):
    i32, i64 = torch.int32, torch.int64
    shape = (rows,) if g == 1 else (rows, g)
    return dict(logits=torch.zeros((rows * g, vocab), dtype=torch.float16, device=device), ids=torch.zeros(shape, dtype=i64, device=device),
                pos=torch.zeros(shape, dtype=i64, device=device), seen=torch.zeros((rows, stride), dtype=i32, device=device),
                n_prompt=torch.zeros(rows, dtype=i32, device=device), repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25,
                workspace=torch.zeros(rows * vocab, dtype=i32, device=device))


def test_cpu_tensors_raise_and_values_are_checked():
    import qqq_amd
    from qqq_amd import ops

    assert qqq_amd.penalize_logits is ops.penalize_logits and "penalize_logits" in qqq_amd.__all__
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.penalize_logits(**_op_args())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.penalize_logits(**dict(_op_args(), workspace=None))
    with pytest.raises(RuntimeError, match="presence_penalty holds 2 entries"):
        ops.penalize_logits(**dict(_op_args(), presence_penalty=torch.ones(2)))
    with pytest.raises(RuntimeError, match=r"fp16 \[rows \* group, vocab\] tensor"):
        ops.penalize_logits(**dict(_op_args(), logits=torch.zeros(40, dtype=torch.float16)))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="repetition_penalty=.* must be finite and > 0"):
            ops.penalize_logits(**dict(_op_args(), repetition_penalty=bad))


def test_fake_implementation_checks_dtypes_and_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from qqq_amd import ops

    i32, i64 = torch.int32, torch.int64
    with FakeTensorMode():
        a = _op_args()
        assert ops.penalize_logits(**a) is a["logits"]
        a = _op_args(g=1)
        assert ops.penalize_logits(**a) is a["logits"]
        wide = torch.zeros((6, 48), dtype=torch.float16)
        assert ops.penalize_logits(**dict(_op_args(), logits=wide[:, :40])).shape == (6, 40)  # a padded head output, in place
        for bad, msg in ((dict(logits=torch.zeros((6, 40))), "logits must be fp16"), (dict(ids=torch.zeros((3, 2), dtype=i32)), "ids must be int64"),
                         (dict(ids=torch.zeros((3, 17), dtype=i64)), "group <= 16"), (dict(logits=torch.zeros((8, 40), dtype=torch.float16)), "logits hold 8 rows"),
                         (dict(pos=torch.zeros(3, dtype=i64)), "pos must be int64"), (dict(pos=torch.zeros((3, 2), dtype=i32)), "pos must be int64"),
                         (dict(seen=torch.zeros((3, 9), dtype=i64)), "seen must be int32"), (dict(seen=torch.zeros((2, 9), dtype=i32)), "seen"),
                         (dict(seen=torch.zeros((3, 0), dtype=i32)), "seen_stride >= 1"), (dict(n_prompt=torch.zeros(3, dtype=i64)), "n_prompt must be int32"),
                         (dict(n_prompt=torch.zeros(4, dtype=i32)), "n_prompt"), (dict(workspace=torch.zeros(119, dtype=i32)), "workspace must be int32"),
                         (dict(workspace=torch.zeros(120)), "workspace"),
                         (dict(logits=torch.zeros((40, 6), dtype=torch.float16).t()), "rewritten in place, never copied"),
                         (dict(logits=torch.zeros((6, 80), dtype=torch.float16)[:, ::2]), "never copied")):
            with pytest.raises(RuntimeError, match=msg):
                ops.penalize_logits(**dict(_op_args(), **bad))
        with pytest.raises(RuntimeError, match="outside 1 <= vocab <= 262144"):
            ops.penalize_logits(**_op_args(rows=1, g=1, vocab=262145))
        with pytest.raises(RuntimeError, match=r"rows \* group <= 65535"):
            ops.penalize_logits(**_op_args(rows=4096, g=16, vocab=8))


# ---- the loops' bookkeeping, with host stubs for the forward pass and the ops

def _stub_penalize(calls):
    """ops.penalize_logits on the loops' own CPU arrays through penalty_ref, recording (rows, group, what the parameters were)"""

    def penalize(logits, ids, pos, seen, n_prompt, rep, pres, freq, workspace=None):
        as_np = lambda v: v.numpy() if isinstance(v, torch.Tensor) else v  # noqa: E731
        calls.append((ids.shape[0], 1 if ids.dim() == 1 else ids.shape[1], np.array(as_np(rep)).tolist()))
        assert workspace is not None and workspace.dtype == torch.int32 and workspace.numel() >= ids.shape[0] * logits.shape[1]
        assert not workspace.any()
        got, seen2 = penalty_ref.penalize(logits.numpy(), ids.numpy(), pos.numpy(), seen.numpy(), n_prompt.numpy(), as_np(rep), as_np(pres),
                                          as_np(freq))
        logits.copy_(torch.from_numpy(got))
        seen.copy_(torch.from_numpy(seen2))
        return logits

    return penalize


STATE = ("ids", "pos", "slots", "block_table", "remaining", "eos", "n_out", "tick", "u", "temperature", "top_k", "top_p")


def test_decode_loop_with_penalties_over_host_stubs(monkeypatch):
    """The stub model's greedy token is (t + 1) % 50, with logit 1 on it and 0 elsewhere.  A presence penalty of 2 on a loop whose prompt
    already holds the next tokens changes nothing while they are prompt tokens only (presence counts outputs), and sends the argmax to
    token 0 -- the lowest index of the maximum 0 -- once the successor has been emitted before."""
    from qqq_amd import DecodeLoop
    from test_step_cpu import _LoopStub, _run_up, _tiny_lm

    m = _tiny_lm()
    stub = _LoopStub(m, monkeypatch)
    calls = []
    monkeypatch.setattr("qqq_amd.serve.ops.penalize_logits", _stub_penalize(calls))
    cache = m.new_cache(6, 16)
    plain = DecodeLoop(m, cache, rows=2, max_len=48, sync_every=3, u_stride=4, graph=False)
    assert not plain.penalties and not any(hasattr(plain, a) for a in ("seen", "n_prompt", "repetition", "presence", "frequency", "penalty_workspace"))
    prompts = [[1, 2, 3], [10] * 17, [7]]
    want = plain.generate(prompts, 9)
    assert want == [_run_up(4, 9), _run_up(11, 9), _run_up(8, 9)] and calls == []  # neutral: no call, nothing new allocated
    assert not hasattr(plain, "seen")
    # non-neutral values on a loop without the flag: refused before anything runs
    passes, prefills = stub.decode_passes, list(stub.prefills)
    for kw in (dict(repetition_penalty=1.3), dict(presence_penalty=0.5), dict(frequency_penalty=-0.25)):
        with pytest.raises(ValueError, match="need a loop built with penalties=True"):
            plain.generate(prompts, 9, **kw)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="must be finite and > 0"):
            plain.generate(prompts, 9, repetition_penalty=bad)
    assert stub.decode_passes == passes and stub.prefills == prefills and cache.free_blocks == 6 and calls == []

    loop = DecodeLoop(m, cache, rows=2, max_len=48, sync_every=3, u_stride=4, graph=False, penalties=True)
    assert loop.penalties and loop.seen.shape == (2, 48) and loop.seen.dtype == torch.int32 and loop.penalty_workspace.shape == (2 * 50,)
    assert loop.repetition.tolist() == [1, 1] and loop.presence.tolist() == [0, 0] and loop.frequency.tolist() == [0, 0]
    for a in STATE:
        assert getattr(loop, a).shape == getattr(plain, a).shape and getattr(loop, a).dtype == getattr(plain, a).dtype
    # neutral values on a loop with the flag: the op rides in every step (it keeps `seen`), the tokens are the plain loop's
    assert loop.generate(prompts, 9) == want and calls and all(c[2] == [1.0, 1.0] for c in calls) and all(c[1] == 1 for c in calls)
    # row 0 served the first prompt and then the third: the prompt from admission, every fed token recorded by the op (the last emitted
    # token is never fed)
    assert loop.seen[0, :9].tolist() == [7] + _run_up(8, 8) and loop.n_prompt.tolist() == [1, 17]
    # presence 2 over the prompt [48, 49, 0, 1]: the successor's logit 1 stands while the successor was never EMITTED (0 and 1 are prompt
    # tokens: no output occurrence), so the tokens run 2 ... 49, 0, 1 -- all 50, each once
    del calls[:]
    got = loop.generate([[48, 49, 0, 1]], 44, presence_penalty=2.0)[0]
    assert got == list(range(2, 46)) and calls[0] == (1, 1, 1.0)  # the admission call: one row, over the prompt
    long = DecodeLoop(m, cache, rows=1, max_len=64, sync_every=4, u_stride=4, graph=False, penalties=True)
    got = long.generate([[48, 49, 0, 1]], 52, presence_penalty=2.0)[0]
    assert got[:50] == list(range(2, 50)) + [0, 1] and long.seen[0, :54].tolist() == [48, 49, 0, 1] + got[:50]
    # ... and then the successor 2 has been emitted: 1 - 2 = -1 loses to the zeros of the tokens never emitted -- there are none left,
    # every token stands at -2 or (the successor) -1: the successor still wins
    assert got[50:] == [2, 3]
    assert long.n_prompt.tolist() == [4] and long.presence.tolist() == [2.0] and cache.free_blocks == 6
    # reuse with neutral values: the plain loop's tokens again
    assert long.generate([[7]], 9) == [_run_up(8, 9)] and long.presence.tolist() == [0.0]


def test_spec_loop_with_penalties_over_host_stubs(monkeypatch):
    from qqq_amd import SpecDecodeLoop
    from test_spec_cpu import MOD, _count_up, _LoopStub, _tiny_lm

    m = _tiny_lm()
    stub = _LoopStub(m, monkeypatch)
    calls = []
    monkeypatch.setattr("qqq_amd.serve.ops.penalize_logits", _stub_penalize(calls))
    cache = m.new_cache(6, 16)
    plain = SpecDecodeLoop(m, cache, rows=2, max_len=48, draft_len=3, sync_every=3, graph=False)
    want = plain.generate([[1, 2, 3], [4]], 9)
    assert want == [_count_up(4, 9), _count_up(0, 9)] and calls == [] and not hasattr(plain, "seen") and not hasattr(plain, "n_prompt")
    passes = stub.passes
    with pytest.raises(ValueError, match="need a loop built with penalties=True"):
        plain.generate([[1, 2, 3]], 9, frequency_penalty=0.5)
    assert stub.passes == passes and cache.free_blocks == 6
    loop = SpecDecodeLoop(m, cache, rows=2, max_len=48, draft_len=3, sync_every=3, graph=False, penalties=True)
    assert loop.seen is loop.hist and loop.penalty_workspace.shape == (2 * 50,)
    assert loop.generate([[1, 2, 3], [4]], 9) == want and calls and all(c[1] == 4 for c in calls)
    # a repetition penalty leaves the one-hot argmax where it is (1 / 1.5 > 0): the same tokens, the parameters written per admitted row
    del calls[:]
    assert loop.generate([[1, 2, 3], [4]], 9, repetition_penalty=1.5) == want
    assert calls[0] == (2, 1, 1.5) and all(c[1:] == (4, [1.5, 1.5]) for c in calls[1:]) and loop.n_prompt.tolist() == [3, 1]
    # presence 2 makes every emitted token lose against the lowest unemitted one: tokens never repeat while MOD allows
    got = loop.generate([[1]], 4, presence_penalty=2.0)[0]
    assert got == [2, 3, 4, 0] and len(set(got)) == 4 and MOD == 5


def test_generate_passes_penalties_on_only_when_they_are_set(monkeypatch):
    from test_step_cpu import _tiny_lm

    m = _tiny_lm()
    made = []

    class _Loop:
        def __init__(self, lm, cache, rows, max_len, *a, **kw):
            made.append((a, kw))

        def generate(self, *a, **kw):
            return ["delegated", a, kw]

    monkeypatch.setattr("qqq_amd.serve.DecodeLoop", _Loop)
    monkeypatch.setattr("qqq_amd.serve.SpecDecodeLoop", _Loop)
    prompts = [[1, 2, 3], [4] * 20]
    args = (prompts, 9, 0.5, 7, 0.9, None, 3)
    assert m.generate(*args, device_loop=True, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0) == ["delegated", args, {}]
    assert m.generate(*args, device_loop=True, draft_len=5) == ["delegated", args, {}]
    assert made == [((), {}), ((), dict(draft_len=5))]
    pen = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.25)
    assert m.generate(*args, device_loop=True, **pen) == ["delegated", args, pen]
    assert m.generate(*args, device_loop=True, draft_len=5, **pen) == ["delegated", args, pen]
    assert made[2:] == [((), dict(penalties=True)), ((), dict(draft_len=5, penalties=True))]
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="repetition_penalty=.* must be finite and > 0"):
            m.generate(*args, repetition_penalty=bad)
    # the keywords follow draft_len
    import inspect

    names = list(inspect.signature(m.generate).parameters)
    assert names[names.index("draft_len") + 1:] == ["repetition_penalty", "presence_penalty", "frequency_penalty"]


def test_host_loop_penalises_every_pass_through_the_op(monkeypatch):
    from test_step_cpu import _LoopStub, _run_up, _tiny_lm

    m = _tiny_lm()
    _LoopStub(m, monkeypatch)
    calls = []
    monkeypatch.setattr("qqq_amd.model.ops.sample_tokens", lambda logits, T, k, p, u: logits.argmax(dim=1))
    monkeypatch.setattr("qqq_amd.model.ops.penalize_logits", _stub_penalize(calls))
    assert m.generate([[1, 2, 3], [7]], 5) == [_run_up(4, 5), _run_up(8, 5)] and calls == []
    got = m.generate([[48, 49, 0, 1], [7]], 6, presence_penalty=2.0)
    assert got == [list(range(2, 8)), _run_up(8, 6)] and len(calls) == 6 and calls[0][:2] == (2, 1)
    # the successor of 1 is 2, emitted before: it loses to the lowest index at the maximum
    assert m.generate([[5, 0]], 4, presence_penalty=2.0, repetition_penalty=1.0) == [[1, 2, 3, 4]]
    assert m.generate([[49]], 3, presence_penalty=2.0) == [[0, 1, 2]]
    assert m.generate([[2]], 4, eos_token_id=4, frequency_penalty=2.0) == [[3, 4]]
