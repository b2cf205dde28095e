"""Scoring without a GPU: tests/score_ref.py against torch.log_softmax in float64, pack_steps on hand-worked cases, the perplexity
convention on made-up log-probs, the C-ABI of include/qqq_amd_score.h (declared set, export, argument checks before any launch, the NULL
no-op), the kernel's resources in the gfx950 code object, and the op's CPU refusal and fake implementation."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from score_ref import token_logprob_row, token_logprobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 17


# ---- the reference against torch.log_softmax in float64

def _torch_ref(l, t):
    return float(torch.log_softmax(torch.from_numpy(np.asarray(l).astype(np.float64)), -1)[t])


@pytest.mark.parametrize("vocab", [1, 7, 65, 1001])
@pytest.mark.parametrize("scale", [0.5, 4.0, 30.0])
def test_reference_equals_log_softmax_in_float64(vocab, scale):
    rng = np.random.default_rng(vocab * 31 + int(scale * 2))
    l = (scale * rng.standard_normal((4, vocab))).astype(np.float16)
    for row in l:
        for t in {0, vocab - 1, int(row.argmax()), int(row.argmin())}:
            got, am = token_logprob_row(row, t)
            assert abs(got - _torch_ref(row, t)) <= 1e-12 * max(1.0, abs(got))
            assert am == int(torch.from_numpy(row.astype(np.float64)).argmax())
    lp, am = token_logprobs(l, [0, vocab - 1, 0, vocab - 1])
    assert lp.shape == (4,) and am.dtype == np.int64 and lp[1] == token_logprob_row(l[1], vocab - 1)[0]


def test_reference_special_cases():
    l = np.array([0.5, 2.0, -np.inf, 2.0, np.nan, -1.0], np.float16)
    clean = np.where(np.isnan(l.astype(np.float64)), -np.inf, l.astype(np.float64))  # what log_softmax can be asked instead
    # ignored targets
    assert token_logprob_row(l, -1) == (0.0, 1) and token_logprob_row(l, -100) == (0.0, 1)
    # out of range
    for t in (6, 7, 1 << 40):
        got, am = token_logprob_row(l, t)
        assert math.isnan(got) and am == 1
    # NaN or -inf at the target
    assert token_logprob_row(l, 2)[0] == -math.inf and token_logprob_row(l, 4)[0] == -math.inf
    # NaN and -inf have no weight: the other targets are log_softmax of the row with them at -inf
    for t in (0, 1, 3, 5):
        assert abs(token_logprob_row(l, t)[0] - _torch_ref(clean, t)) <= 1e-12
    assert abs(token_logprob_row(l, 1)[0] - (-math.log(2 + math.exp(-1.5) + math.exp(-3.0)))) <= 1e-12
    # +inf as the maximum: its tie group shares the mass, finite targets get -inf; log_softmax of (0 in the group, -inf elsewhere) says the same
    p = l.copy()
    p[[0, 3, 5]] = np.inf
    group = np.where(np.isposinf(p.astype(np.float64)), 0.0, -np.inf)
    for t in (0, 3, 5):
        got, am = token_logprob_row(p, t)
        assert abs(got + math.log(3)) <= 1e-15 and am == 0 and abs(got - _torch_ref(group, t)) <= 1e-12
    assert token_logprob_row(p, 1)[0] == -math.inf == _torch_ref(group, 1) and token_logprob_row(p, 4)[0] == -math.inf
    # a row without any logit above -inf
    for fill in (-np.inf, np.nan):
        e = np.full(5, fill, np.float16)
        got, am = token_logprob_row(e, 2)
        assert math.isnan(got) and am == 0
        assert token_logprob_row(e, -1) == (0.0, 0) and math.isnan(token_logprob_row(e, 5)[0])
    # -0 equals +0: the lowest index wins, and the two share the maximum
    z = np.array([-3.0, -0.0, 0.0, -2.0], np.float16)
    for t in (1, 2):
        got, am = token_logprob_row(z, t)
        assert am == 1 and abs(got - _torch_ref(z, t)) <= 1e-12
    # a target so far below the maximum that its own weight vanishes still has its log-probability
    far = np.array([60000.0, -60000.0, 0.0], np.float16)
    assert token_logprob_row(far, 1)[0] == float(np.float16(-60000.0)) - float(np.float16(60000.0)) and token_logprob_row(far, 0)[0] == 0.0


# ---- pack_steps

def _check_plan(lengths, chunk, bs, steps, blocks):
    from qqq_amd.score import pack_steps

    got_steps, got_blocks = pack_steps(lengths, chunk, bs)
    assert got_steps == steps and got_blocks == blocks
    # token counts are conserved: every sequence is covered once, in order, and no step is over-full; all but the last are full
    at = [0] * len(lengths)
    for n, step in enumerate(got_steps):
        assert 1 <= sum(c for _, _, c in step) <= chunk and (n == len(got_steps) - 1 or sum(c for _, _, c in step) == chunk)
        assert [i for i, _, _ in step] == sorted({i for i, _, _ in step})
        for i, start, count in step:
            assert start == at[i] and count >= 1
            at[i] += count
    assert at == list(lengths)
    # the per-step block need, replayed with an allocator of one's own: add at the first chunk, free after the last
    held = {}
    for step, want in zip(got_steps, got_blocks):
        for i, start, count in step:
            held[i] = -(-(start + count) // bs)
        assert sum(held.values()) == want
        for i, start, count in step:
            if start + count == lengths[i]:
                del held[i]
    assert not held


def test_pack_steps_hand_worked_cases():
    # an exact fit: two sequences fill one step; a sequence that ends where the step fills
    _check_plan([8, 8], 16, 16, [[(0, 0, 8), (1, 0, 8)]], [2])
    _check_plan([16, 4], 16, 16, [[(0, 0, 16)], [(1, 0, 4)]], [1, 1])
    # a split in the middle of a sequence
    _check_plan([10, 10], 16, 16, [[(0, 0, 10), (1, 0, 6)], [(1, 6, 4)]], [2, 1])
    # one sequence over three steps: it holds one block more in each
    _check_plan([40], 16, 16, [[(0, 0, 16)], [(0, 16, 16)], [(0, 32, 8)]], [1, 2, 3])
    # many short sequences in one step: a block each
    _check_plan([3, 1, 2, 5, 4], 16, 16, [[(0, 0, 3), (1, 0, 1), (2, 0, 2), (3, 0, 5), (4, 0, 4)]], [5])
    # chunk_tokens = 1: a token per step
    _check_plan([2, 1], 1, 16, [[(0, 0, 1)], [(0, 1, 1)], [(1, 0, 1)]], [1, 1, 1])
    # the model tests' prompts at 16 tokens per step: splits inside and across the sequences
    _check_plan([5, 17, 33], 16, 16, [[(0, 0, 5), (1, 0, 11)], [(1, 11, 6), (2, 0, 10)], [(2, 10, 16)], [(2, 26, 7)]], [2, 3, 2, 3])
    _check_plan([5, 17, 33], 64, 16, [[(0, 0, 5), (1, 0, 17), (2, 0, 33)]], [6])
    # another block size
    _check_plan([40, 3], 32, 32, [[(0, 0, 32)], [(0, 32, 8), (1, 0, 3)]], [1, 3])
    _check_plan([], 8, 16, [], [])


def test_pack_steps_refuses_bad_arguments():
    from qqq_amd.score import pack_steps

    for lengths, chunk in (([3, 0], 8), ([3], 0), ([-1], 4)):
        with pytest.raises(ValueError, match="pack_steps"):
            pack_steps(lengths, chunk)


# ---- the perplexity convention

def test_perplexity_is_the_reference_convention_on_made_up_logprobs():
    from qqq_amd.score import perplexity_from_logprobs

    seqlen = 5
    windows = [[-1.0, -2.0, -3.0, -2.0], [-0.5, -0.5, -0.5, -0.5], [-4.0, 0.0, 0.0, 0.0]]
    # per window: mean over the seqlen - 1 targets, times seqlen; exp(sum / (nsamples * seqlen))
    nll = [2.0 * seqlen, 0.5 * seqlen, 1.0 * seqlen]
    want = math.exp(sum(nll) / (3 * seqlen))
    assert want == math.exp(3.5 / 3)
    got = perplexity_from_logprobs([torch.tensor(w) for w in windows], seqlen)
    assert abs(got - want) <= 1e-12 * want
    # the same through torch's CrossEntropyLoss, as the reference forms it: logits whose log_softmax at the label is the made-up log-prob
    nlls = []
    for w in windows:
        lp = torch.tensor(w, dtype=torch.float64)
        logits = torch.stack([lp, torch.log1p(-torch.exp(lp).clamp(max=1 - 1e-12))], 1)  # two classes: p and 1 - p
        loss = torch.nn.CrossEntropyLoss()(logits, torch.zeros(seqlen - 1, dtype=torch.int64))
        nlls.append(loss * seqlen)
    ref = float(torch.exp(torch.stack(nlls).sum() / (3 * seqlen)))
    assert abs(got - ref) <= 1e-9 * ref
    # every window has seqlen - 1 targets: another length raises
    with pytest.raises(ValueError, match="targets"):
        perplexity_from_logprobs([torch.zeros(seqlen)], seqlen)
    # the factor seqlen of the per-window nll cancels against the divisor's: what is left is the mean over the windows' targets, and NOT
    # the total nll over the total number of tokens
    flat = -sum(sum(w) for w in windows)
    assert abs(got - math.exp(flat / (3 * (seqlen - 1)))) <= 1e-12 * got and abs(got - math.exp(flat / (3 * seqlen))) > 0.1


# ---- the C-ABI

@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def test_header_declares_the_entry_and_the_library_exports_it(L):
    from qqq_amd import _abi

    names = set(_abi.prototypes(os.path.join(ROOT, "include", "qqq_amd_score.h")))
    assert names == {"qqq_token_logprobs"}
    assert hasattr(L, "qqq_token_logprobs") and L.qqq_amd_abi_version() == 4
    main = _abi.source(os.path.join(ROOT, "include", "qqq_amd.h"))
    assert "qqq_token_logprobs" not in main  # the feature has its own header (a newer one rebuilds the library: tests/test_abi_cpu.py)


# fake device addresses with the alignment the entry point asks for: the calls below must fail in the checks, before any launch
A16, A8, A4 = 0x10000, 0x20008, 0x30004


def _call(L, logits=A16, ld=32000, targets=A8, logprob=A4, argmax=A8 + 64, rows=4, vocab=32000):
    return L.qqq_token_logprobs(logits, ld, targets, logprob, argmax, rows, vocab, 0, None)


BAD = [dict(logits=None), dict(targets=None), dict(logprob=None), dict(logits=A16 + 8), dict(logits=A16 + 2), dict(targets=A8 + 4),
       dict(logprob=A4 + 2), dict(logprob=A4 + 1), dict(argmax=A8 + 4), dict(argmax=A8 + 1), dict(ld=31999), dict(ld=31992),
       dict(vocab=1001, ld=1001), dict(vocab=1001, ld=1004), dict(vocab=1001, ld=1000), dict(vocab=0, ld=8), dict(vocab=0, ld=0),
       dict(vocab=-1, ld=8), dict(vocab=262145, ld=262152), dict(rows=-1), dict(rows=1048577)]


@pytest.mark.parametrize("kw", BAD)
def test_token_logprobs_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _call(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_token_logprobs")


def test_rows_0_is_a_no_op_with_null_pointers(L):
    z = None
    assert L.qqq_token_logprobs(z, 0, z, z, z, 0, 32000, 0, z) == 0
    assert L.qqq_token_logprobs(z, 0, z, z, z, 0, 0, 0, z) == 0
    assert _call(L, rows=0) == 0


def test_score_kernel_in_the_code_object_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB) if "logprobs" in k["demangled"]}
    assert set(ks) == {"qqq_token_logprobs_kernel"}
    for k in ks.values():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        # sixteen waves; registers leave room for two workgroups per CU (128 registers per lane); two 128-byte arrays of LDS
        assert k["max_flat_workgroup_size"] == 1024 and k["vgpr_count"] + k["agpr_count"] <= 128 and k["group_segment_fixed_size"] <= 1024, k


# ---- the op

def test_cpu_tensors_and_bad_shapes_raise():
    import qqq_amd
    from qqq_amd import ops

    assert qqq_amd.token_logprobs is ops.token_logprobs
    logits = torch.zeros((3, 40), dtype=torch.float16)
    t = torch.zeros(3, dtype=torch.int64)
    for fn in (ops.token_logprobs, ops._token_logprobs_impl) + ((ops._ext().token_logprobs,) if ops._ext() is not None else ()):
        with pytest.raises(RuntimeError, match="token_logprobs: .*no CPU path"):
            fn(logits, t, True)
    with pytest.raises(RuntimeError, match=r"^token_logprobs: logits must be"):
        ops.token_logprobs(logits[0], t)
    with pytest.raises(RuntimeError, match=r"^token_logprobs: logits must be"):
        ops.token_logprobs([[0.0]], t)
    for bad_logits, bad_t in ((logits.float(), t), (logits, t.int()), (logits, t[:2]), (logits, t[None]),
                              (torch.zeros((3, 0), dtype=torch.float16), t)):
        with pytest.raises(RuntimeError, match=r"^token_logprobs: "):
            ops._token_logprobs_check(bad_logits, bad_t)


def test_fake_implementation_gives_f32_and_int64_rows():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from qqq_amd import ops

    with FakeTensorMode():
        logits = torch.empty((9, 32000), dtype=torch.float16)
        t = torch.empty(9, dtype=torch.int64)
        lp, am = torch.ops.qqq_amd.token_logprobs(logits, t, True)
        assert lp.shape == (9,) and lp.dtype == torch.float32 and am.shape == (9,) and am.dtype == torch.int64
        lp, am = ops.token_logprobs(logits, t)
        assert lp.shape == (9,) and lp.dtype == torch.float32 and am.shape == (9,) and am.dtype == torch.int64
        lp, am = ops.token_logprobs(logits[:, :31999], t, return_argmax=False)
        assert lp.shape == (9,) and am is None


def test_model_methods_delegate_to_the_scoring_module():
    from qqq_amd import QuantLlamaForCausalLM, pack_steps, score

    assert pack_steps is score.pack_steps
    for name in ("score", "loglikelihood", "perplexity"):
        assert callable(getattr(QuantLlamaForCausalLM, name)) and callable(getattr(score, name))
