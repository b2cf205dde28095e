"""The speculative decode loop's step without a GPU: tests/spec_ref.py's draft rule against serve.ngram_draft, the algorithm's property (the
speculative loop emits exactly the plain greedy sequence), the C-ABI of include/qqq_amd_spec.h (declared set, exports, argument checks
before any launch, the NULL no-op), the kernels' resources in the gfx950 code object, the op's CPU refusal and fake implementation, and
SpecDecodeLoop's bookkeeping over host stubs."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import spec_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 17
BS = 16


# ---- the draft rule

@pytest.mark.parametrize("alphabet", [2, 3, 5])
def test_reference_draft_equals_ngram_draft_over_random_histories(alphabet):
    from qqq_amd.serve import ngram_draft

    rng = np.random.default_rng(alphabet)
    matched = {n: 0 for n in range(5)}
    for length in range(1, 41):
        for _ in range(4):
            h = rng.integers(0, alphabet, length).tolist()
            for k, nmax in itertools.product((1, 3, 15), (1, 2, 3, 4)):
                want = spec_ref.draft(h, k, nmax)
                assert ngram_draft(h, k, nmax) == want and len(want) == k, (h, k, nmax)
            deepest = max([n for n in range(1, 5) if n < length and any(h[i:i + n] == h[length - n:] for i in range(length - n))], default=0)
            matched[deepest] += 1
    assert all(matched[n] for n in range(5)), matched  # every depth of match, and no match at all, occurred


def test_draft_rule_cases():
    from qqq_amd.serve import ngram_draft

    for f in (spec_ref.draft, ngram_draft):
        assert f([4], 3, 3) == [4, 4, 4]                      # n < L leaves no n: the last token repeats
        assert f([1, 2, 3], 2, 3) == [3, 3]                    # no match
        assert f([1, 2, 3, 1, 2], 4, 3) == [3, 1, 2, 3]        # the 2-gram at 0; the copy runs over the end and goes on with its own output
        assert f([1, 2, 1, 2, 1], 6, 3) == [2, 1, 2, 1, 2, 1]  # the overlapping copy: the 3-gram at 0 overlaps the tail
        assert f([7, 7], 5, 4) == [7] * 5                      # a period of one
        assert f([1, 2, 9, 3, 2, 8, 4, 2], 2, 3) == [8, 4]     # the largest i wins: the later of the two 2s
        assert f([1, 2, 3, 9, 2, 3, 8, 3], 2, 1) == [8, 3]     # ngram_max 1 takes the latest 3 ...
        assert f([1, 2, 3, 9, 2, 3, 8, 2, 3], 2, 2) == [8, 2]  # ... and the longer n-gram is preferred to a later shorter one
        assert f([5, 1, 2, 3, 4, 6, 1, 2, 3, 4], 3, 4) == [6, 1, 2]
        assert f([5, 1, 2, 3, 4, 6, 0, 2, 3, 4], 3, 4) == [6, 0, 2]  # the 4-gram fails, the 3-gram matches
    with pytest.raises(ValueError):
        ngram_draft([], 3, 3)


# ---- the algorithm: speculation changes no token

def _next_token(history):
    """the toy model: a hash of the last three tokens, mod 5"""
    a, b, c = ([0, 0, 0] + [int(t) for t in history])[-3:]
    return (a * 31 + b * 17 + c * 7 + (a * b + c) % 11 + 3) % 5


def _plain(prompt, n_new, eos=-1):
    h, out = list(prompt), []
    while len(out) < n_new:
        out.append(_next_token(h))
        h.append(out[-1])
        if out[-1] == eos:
            break
    return out


def _speculative(prompt, n_new, k, nmax, eos=-1):
    """-> (the tokens, the accepted drafts of every step).  The first token comes from the prefill; every later step scores the row's
    last token and its k drafts with the toy model and hands the draws to spec_ref.advance."""
    first = _next_token(prompt)
    if n_new == 1 or first == eos:
        return [first], []
    st = spec_ref.new_state(1, k, 16, 200, BS)
    spec_ref.seat(st, 0, list(prompt) + [first], list(range(16)), n_new - 1, nmax, eos)
    accepted = []
    while st["remaining"][0] > 0:
        n = int(st["hist_len"][0])
        assert st["hist"][0, n - 1] == st["ids"][0, 0] and st["pos"][0, 0] == st["start"][0] == n - 1
        h = st["hist"][0, :n].tolist()
        draws = [_next_token(h + st["ids"][0, 1:1 + j].tolist()) for j in range(k + 1)]  # draw j saw the drafts before it
        before = int(st["n_acc"][0])
        spec_ref.advance(st, [draws], nmax)
        accepted.append(int(st["n_acc"][0]) - before)
    n, m = int(st["hist_len"][0]), int(st["n_out"][0])
    assert m == sum(accepted) + len(accepted)  # a step emits one token more than it accepts drafts
    return [first] + st["hist"][0, n - m:n].tolist(), accepted


def test_speculative_loop_emits_the_plain_greedy_sequence():
    prompts = ([1], [0, 2], [1, 2], [3, 1, 4, 1, 0, 2], [0, 0, 0, 0], [2, 4, 2, 4, 2, 4, 2])
    full = none = eos_mid = False
    for prompt, k, nmax, n_new in itertools.product(prompts, (1, 2, 3, 7, 15), (1, 2, 3, 4), (1, 2, 30, 61)):
        want = _plain(prompt, n_new)
        got, accepted = _speculative(prompt, n_new, k, nmax)
        assert got == want and len(got) == n_new, (prompt, k, nmax, n_new)
        full |= k in accepted
        none |= 0 in accepted
        # every token of the run as the eos: the sequence ends with its first occurrence, in the middle of a chunk or not
        for eos in sorted(set(want)):
            cut = want[:want.index(eos) + 1]
            got, accepted = _speculative(prompt, n_new, k, nmax, eos)
            assert _plain(prompt, n_new, eos) == cut and got == cut, (prompt, k, nmax, n_new, eos)
            # the eos was draw j >= 1 of its step, behind accepted drafts, and the budget was not what ended the run
            eos_mid |= len(cut) < n_new and bool(accepted) and accepted[-1] >= 1
    assert full and none  # the drafter was right K times in one step at least once, and wrong at once at least once
    assert eos_mid       # and an eos ended a sequence in the middle of a chunk


def test_budget_ends_a_chunk_in_its_middle():
    # a period of one ([0, 0, 0] -> 3, then the toy model settles): find a run whose drafts are all accepted, and cut it mid-chunk
    prompt, k, nmax = [2, 4, 2, 4, 2, 4, 2], 7, 3
    want = _plain(prompt, 61)
    got, accepted = _speculative(prompt, 61, k, nmax)
    assert got == want and k in accepted
    first_full = accepted.index(k)
    emitted_before = 1 + sum(a + 1 for a in accepted[:first_full])
    for extra in (1, 2, k):  # the budget ends 1, 2, k tokens into the chunk that would have emitted k + 1
        n_new = emitted_before + extra
        got, acc = _speculative(prompt, n_new, k, nmax)
        assert got == want[:n_new] and acc[:first_full] == accepted[:first_full] and acc[first_full] == extra - 1


def test_reference_retires_instead_of_leaving_hist_or_the_table():
    k, nmax = 3, 2
    st = spec_ref.new_state(3, k, 2, 12, BS)
    spec_ref.seat(st, 0, [1, 2, 1, 2, 1, 2, 1, 2, 1], [5, 6], 100, nmax)  # hist holds 12: three more tokens fit
    spec_ref.seat(st, 1, [1, 2, 1, 2, 1, 2, 1, 2, 1], [7, 8], 100, nmax)
    st["hist_len"][1] = 12                                               # state no caller reaches: an active row without room
    spec_ref.seat(st, 2, [3] * 11, [1, 2], 100, nmax)                    # one more token fits
    assert st["ids"][0].tolist() == [1, 2, 1, 2]
    before = spec_ref.copy_state(st)
    spec_ref.advance(st, [[2, 1, 2, 1], [4, 4, 4, 4], [3, 3, 3, 3]], nmax)
    # row 0: every draft is right, but hist is full after three appends: the fourth is not made, and the row retires
    assert st["hist_len"][0] == 12 and st["hist"][0].tolist() == [1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2]
    assert st["n_out"][0] == 3 and st["n_acc"][0] == 3
    assert st["remaining"][0] == 0 and (st["pos"][0] == -1).all() and st["start"][0] == -1 and (st["ids"][0] == 0).all()
    # row 1: nothing is appended
    assert np.array_equal(st["hist"][1], before["hist"][1]) and st["n_out"][1] == 0 and st["hist_len"][1] == 12
    assert st["remaining"][1] == 0 and st["start"][1] == -1
    # row 2: one token, which fills hist
    assert st["remaining"][2] == 0 and st["n_out"][2] == 1 and st["hist_len"][2] == 12 and st["n_acc"][2] == 1
    assert st["tick"].tolist() == [1, 1, 1]
    # the table: p' + k must stay inside table_stride blocks
    st = spec_ref.new_state(1, k, 2, 64, BS)
    spec_ref.seat(st, 0, list(range(27)), [4, 9], 100, nmax)  # p = 26; after one token p' = 27, p' + 3 = 30: fine; after two, 31: fine
    spec_ref.advance(st, [[50, 51, 52, 53]], nmax)
    assert st["start"][0] == 27 and st["pos"][0].tolist() == [27, 28, 29, 30] and st["slots"][0].tolist() == [9 * 16 + 11 + j for j in range(4)]
    spec_ref.advance(st, [[60, 61, 62, 63]], nmax)
    assert st["start"][0] == 28 and st["slots"][0, 3] == 9 * 16 + 15
    spec_ref.advance(st, [[70, 71, 72, 73]], nmax)  # p' = 29, p' + 3 = 32: outside
    assert st["remaining"][0] == 0 and st["start"][0] == -1 and st["hist_len"][0] == 30 and st["n_out"][0] == 3


# ---- the C-ABI

@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def test_header_declares_the_entries_and_the_library_exports_them(L):
    from qqq_amd import _abi

    names = set(_abi.prototypes(os.path.join(ROOT, "include", "qqq_amd_spec.h")))
    assert names == {"qqq_spec_advance", "qqq_spec_advance_workspace_bytes"}
    for n in names:
        assert hasattr(L, n), n
    assert L.qqq_amd_abi_version() == 4
    main = _abi.source(os.path.join(ROOT, "include", "qqq_amd.h"))
    assert "qqq_spec" not in main  # the feature has its own header (a newer one rebuilds the library: tests/test_abi_cpu.py)


def test_workspace_bytes(L):
    assert L.qqq_spec_advance_workspace_bytes(6, 3) == 6 * 4 * 8 and L.qqq_spec_advance_workspace_bytes(4095, 15) == 4095 * 16 * 8
    for rows, k in ((0, 3), (-1, 3), (6, 0), (6, 16), (4096, 15), (65535, 1)):
        assert L.qqq_spec_advance_workspace_bytes(rows, k) == 0, (rows, k)


# fake device addresses with the alignment the entry point asks for: the calls below must fail in the checks, before any launch
A16, A8, A4 = 0x10000, 0x20008, 0x30004
PTRS = dict(logits=A16, T=A4, k=A4, p=A4, u=A4, tick=A4, ids=A8, pos=A8, slots=A8, start=A8, table=A4, remaining=A4, eos=A4, hist=A4,
            hist_len=A4, n_out=A4, n_acc=A4, ws=A8)


def _call(L, ld=1008, u_stride=4, table_stride=4, hist_stride=64, ws_bytes=6 * 4 * 8, rows=6, draft_len=3, ngram_max=3, vocab=1003,
          block_size=16, **ptrs):
    a = dict(PTRS, **ptrs)
    return L.qqq_spec_advance(a["logits"], ld, a["T"], a["k"], a["p"], a["u"], u_stride, a["tick"], a["ids"], a["pos"], a["slots"],
                              a["start"], a["table"], table_stride, a["remaining"], a["eos"], a["hist"], hist_stride, a["hist_len"],
                              a["n_out"], a["n_acc"], a["ws"], ws_bytes, rows, draft_len, ngram_max, vocab, block_size, 0, None)


BAD = ([{name: None} for name in PTRS] + [dict(logits=A16 + 8)] + [{name: A8 + 4} for name in ("ids", "pos", "slots", "start", "ws")]
       + [{name: A4 + 2} for name in ("T", "k", "p", "u", "tick", "table", "remaining", "eos", "hist", "hist_len", "n_out", "n_acc")]
       + [dict(block_size=b) for b in (24, 8, 512, 0, -16)]
       + [dict(u_stride=3), dict(u_stride=0), dict(u_stride=-1), dict(table_stride=0), dict(table_stride=-3), dict(hist_stride=0),
          dict(hist_stride=-1)]
       + [dict(draft_len=0), dict(draft_len=-1), dict(draft_len=16), dict(ngram_max=0), dict(ngram_max=5), dict(ngram_max=-2)]
       + [dict(ws_bytes=6 * 4 * 8 - 1), dict(ws_bytes=0), dict(draft_len=15, u_stride=16)]  # the workspace of 3 drafts is short for 15
       + [dict(ld=1003), dict(ld=1000), dict(vocab=0, ld=8), dict(vocab=262145, ld=262152), dict(rows=-1), dict(rows=16384),
          dict(rows=4096, draft_len=15, u_stride=16)])


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_spec_advance_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _call(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_spec_advance:")


def test_rows_0_is_a_no_op_with_null_pointers(L):
    z = None
    assert L.qqq_spec_advance(z, 0, z, z, z, z, 0, z, z, z, z, z, z, 0, z, z, z, 0, z, z, z, z, 0, 0, 3, 3, 1003, 16, 0, z) == 0
    assert L.qqq_spec_advance(z, 0, z, z, z, z, 0, z, z, z, z, z, z, 0, z, z, z, 0, z, z, z, z, 0, 0, 0, 0, 0, 0, 0, z) == 0
    assert _call(L, rows=0) == 0


def test_spec_kernels_in_the_code_object_without_scratch_or_spills():
    """The draw kernel shares the sampler's body and stays inside its budget (sixteen waves, no scratch, its registers and LDS); the advance
    kernel is four waves, a few registers and 80 bytes of LDS.  Neither name touches a family another test enumerates."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB)}
    assert {n for n in ks if "spec" in n} == {"qqq_spec_draw_kernel", "qqq_spec_advance_kernel"}
    draw, adv, smp = ks["qqq_spec_draw_kernel"], ks["qqq_spec_advance_kernel"], ks["qqq_sample_tokens_kernel"]
    for k in (draw, adv):
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert draw["max_flat_workgroup_size"] == 1024 and draw["vgpr_count"] + draw["agpr_count"] <= 128, draw
    assert draw["vgpr_count"] + draw["agpr_count"] <= smp["vgpr_count"] + smp["agpr_count"]
    assert draw["group_segment_fixed_size"] == smp["group_segment_fixed_size"] <= 80 * 1024
    assert adv["max_flat_workgroup_size"] == 256 and adv["vgpr_count"] + adv["agpr_count"] <= 64 and adv["group_segment_fixed_size"] <= 1024


# ---- the op without a GPU

def _op_args(rows=3, k=2, vocab=40, u_stride=6, width=2, hist_stride=9):
    i32, i64, g = torch.int32, torch.int64, k + 1
    return dict(logits=torch.zeros((rows * g, vocab), dtype=torch.float16), temperature=1.0, top_k=0, top_p=1.0,
                u=torch.zeros((rows, u_stride)), tick=torch.zeros(rows, dtype=i32), ids=torch.zeros((rows, g), dtype=i64),
                pos=torch.zeros((rows, g), dtype=i64), slots=torch.zeros((rows, g), dtype=i64), start=torch.zeros(rows, dtype=i64),
                block_table=torch.zeros((rows, width), dtype=i32), remaining=torch.zeros(rows, dtype=i32), eos=torch.zeros(rows, dtype=i32),
                hist=torch.zeros((rows, hist_stride), dtype=i32), hist_len=torch.zeros(rows, dtype=i32), n_out=torch.zeros(rows, dtype=i32),
                n_acc=torch.zeros(rows, dtype=i32), block_size=16, ngram_max=3)


def test_cpu_tensors_raise_and_shapes_are_checked():
    import qqq_amd
    from qqq_amd import ops, serve

    assert qqq_amd.spec_advance is ops.spec_advance and qqq_amd.SpecDecodeLoop is serve.SpecDecodeLoop
    assert qqq_amd.ngram_draft is serve.ngram_draft
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.spec_advance(**_op_args())
    with pytest.raises(RuntimeError, match="temperature holds 2 entries"):
        ops.spec_advance(**dict(_op_args(), temperature=torch.ones(2)))
    with pytest.raises(RuntimeError, match=r"fp16 \[rows \* \(draft_len \+ 1\), vocab\]"):
        ops.spec_advance(**dict(_op_args(), logits=torch.zeros(40, dtype=torch.float16)))


def test_fake_implementation_checks_dtypes_and_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from qqq_amd import ops

    i32, i64 = torch.int32, torch.int64
    with FakeTensorMode():
        assert ops.spec_advance(**_op_args()) is None
        for bad, msg in ((dict(pos=torch.zeros((3, 3), dtype=i32)), "pos must be int64"), (dict(slots=torch.zeros((3, 2), dtype=i64)), "slots"),
                         (dict(tick=torch.zeros(4, dtype=i32)), "tick"), (dict(start=torch.zeros(3, dtype=i32)), "start must be int64"),
                         (dict(u=torch.zeros((3, 2))), "u_stride >= draft_len"), (dict(hist=torch.zeros((3, 9), dtype=i64)), "hist must be int32"),
                         (dict(hist_len=torch.zeros((3, 1), dtype=i32)), "hist_len"), (dict(n_acc=torch.zeros(2, dtype=i32)), "n_acc"),
                         (dict(ids=torch.zeros((3, 1), dtype=i64)), "draft_len <= 15"), (dict(ids=torch.zeros((3, 17), dtype=i64)), "draft_len"),
                         (dict(logits=torch.zeros((8, 40), dtype=torch.float16)), "logits hold 8 rows"),
                         (dict(block_table=torch.zeros((2, 2), dtype=i32)), "block_table"), (dict(block_size=24), "block_size"),
                         (dict(ngram_max=5), "ngram_max"), (dict(ngram_max=0), "ngram_max")):
            with pytest.raises(RuntimeError, match=msg):
                ops.spec_advance(**dict(_op_args(), **bad))


# ---- SpecDecodeLoop: the host's bookkeeping, with host stubs for the forward pass and the two ops

MOD = 5  # the stub model counts up modulo MOD: a period the drafter finds


class _LoopStub:
    """forward: logits whose argmax is (the token + 1) % MOD, for every token of the loop's step and for the last token of each prompt of
    a prefill; sample_tokens: argmax; spec_advance: argmax + spec_ref.advance on the loop's own (CPU) arrays.  Checks every pass's
    positions and slots against the rows' block tables."""

    def __init__(self, m, monkeypatch):
        self.m, self.passes, self.prefills, self.variates = m, 0, [], []
        monkeypatch.setattr(m, "forward", self.forward)
        monkeypatch.setattr("qqq_amd.serve.ops.sample_tokens", lambda logits, T, k, p, u: logits.argmax(dim=1))
        monkeypatch.setattr("qqq_amd.serve.ops.spec_advance", self.advance)

    def forward(self, ids, cache, step, all_rows=False):
        assert ids.dtype == torch.int64 and ids.shape == (sum(step.counts),)
        if all_rows:  # the loop's own step
            g = step.counts[0]
            assert not step.decode and step.counts == [g] * len(step.counts) and step.cu_tokens.tolist() == [g * i for i in range(len(step.counts) + 1)]
            self.passes += 1
            bs = cache.block_size
            pos, slots = step.pos.view(-1, g), step.slots.view(-1, g)
            for r in range(pos.shape[0]):
                if step.start_pos[r] < 0:
                    assert (pos[r] == -1).all() and (slots[r] == -1).all() and (ids.view(-1, g)[r] == 0).all()
                    continue
                assert pos[r].tolist() == list(range(int(step.start_pos[r]), int(step.start_pos[r]) + g)) and pos[r, -1] < step.max_len
                assert slots[r].tolist() == [int(step.block_table[r, p // bs]) * bs + p % bs for p in pos[r].tolist()]
            return torch.nn.functional.one_hot((ids + 1) % MOD, 50).half()
        self.prefills.append(list(step.counts))
        return torch.nn.functional.one_hot((ids[step.cu_tokens[1:].long() - 1] + 1) % MOD, 50).half()

    def advance(self, logits, T, k, p, u, tick, ids, pos, slots, start, block_table, remaining, eos, hist, hist_len, n_out, n_acc, block_size,
                ngram_max):
        g = ids.shape[1]
        assert u.shape[0] * g == logits.shape[0] and (int(tick.max()) + 1) * g <= u.shape[1]  # a variate is never used twice
        self.variates.append(u.view(u.shape[0], -1, g)[torch.arange(u.shape[0]), tick.long()].tolist())
        st = dict(tick=tick.numpy(), ids=ids.numpy(), pos=pos.numpy(), slots=slots.numpy(), start=start.numpy(),
                  block_table=block_table.numpy(), remaining=remaining.numpy(), eos=eos.numpy(), hist=hist.numpy(), hist_len=hist_len.numpy(),
                  n_out=n_out.numpy(), n_acc=n_acc.numpy(), block_size=block_size, draft_len=g - 1)
        spec_ref.advance(st, logits.argmax(dim=1).view(-1, g).tolist(), ngram_max)


def _tiny_lm():
    from test_step_cpu import _tiny_lm as make

    return make().fuse_prefill()


def _count_up(first, n):
    return [(first + j) % MOD for j in range(n)]


def test_spec_loop_bookkeeping_with_host_stubs(monkeypatch):
    from qqq_amd import SpecDecodeLoop

    m = _tiny_lm()
    stub = _LoopStub(m, monkeypatch)
    cache = m.new_cache(6, 16)
    loop = SpecDecodeLoop(m, cache, rows=2, max_len=48, draft_len=3, sync_every=3, graph=False)
    assert loop.u.shape == (2, 12) and loop.ids.shape == loop.pos.shape == loop.slots.shape == (2, 4) and loop.block_table.shape == (2, 3)
    assert loop.step.start_pos is loop.start and loop.step.pos.data_ptr() == loop.pos.data_ptr() and not loop.step.decode
    prompts = [[1, 2, 3], [0] * 17, [2] * 27, [4], [3, 4]]
    # budgets of 14, 28, 38, 12 and 13 keys (9 new tokens, 3 drafts): 1, 2, 3, 1 and 1 blocks through two rows and six blocks
    out = loop.generate(prompts, 9)
    assert out == [_count_up(4, 9), _count_up(1, 9), _count_up(3, 9), _count_up(0, 9), _count_up(0, 9)]
    assert cache.free_blocks == 6 and stub.prefills[0] == [3, 17] and sorted(c for p in stub.prefills for c in p) == [1, 2, 3, 17, 27]
    assert (loop.remaining == 0).all() and (loop.pos == -1).all() and (loop.slots == -1).all() and (loop.start == -1).all()
    assert loop.captures == 0
    # the statistics: 8 tokens per sequence behind the prefill's, one per row-step plus the accepted drafts
    assert loop.row_steps + loop.accepted == 5 * 8 and loop.accepted > 0 and 0 < loop.row_steps < 5 * 8 and loop.steps >= 2
    # one sequence alone: the period shows after MOD + 1 tokens, then every draft is right and a step emits four tokens
    passes = stub.passes
    assert loop.generate([[1]], 21) == [_count_up(2, 21)]
    assert loop.row_steps + loop.accepted == 20 and loop.row_steps < 20 and stub.passes - passes >= loop.row_steps
    # an eos ends a sequence with the eos in its output; a budget of 1 never steps; the rows are reused by the next call
    assert loop.generate(prompts[:2], 9, eos_token_id=1) == [[4, 0, 1], [1]] and cache.free_blocks == 6
    before = stub.passes
    assert loop.generate(prompts, 1) == [[4], [1], [3], [0], [0]] and stub.passes == before
    assert loop.generate(prompts, 0) == [[]] * 5 and loop.generate([], 3) == []


def test_spec_loop_draws_depend_on_the_calls_generator_alone(monkeypatch):
    from qqq_amd import SpecDecodeLoop

    m = _tiny_lm()
    stub = _LoopStub(m, monkeypatch)
    seen = []
    for warm in (False, True):
        loop = SpecDecodeLoop(m, m.new_cache(4, 16), rows=2, max_len=32, draft_len=2, sync_every=2, graph=False)
        if warm:
            loop.generate([[1, 2]], 6)
        stub.variates.clear()
        loop.generate([[1, 2], [3]], 12, temperature=1.0, generator=torch.Generator().manual_seed(5))
        seen.append(list(stub.variates))
    flat = [v for step in seen[0] for row in step for v in row]
    assert seen[0] == seen[1] and len(seen[0]) >= 4 and len(set(flat)) == len(flat)  # u wrapped (2 steps per refill), no variate twice


def test_spec_loop_and_generate_refusals_leave_the_pool_alone(monkeypatch):
    from qqq_amd import SpecDecodeLoop

    m = _tiny_lm()
    stub = _LoopStub(m, monkeypatch)
    cache = m.new_cache(4, 16)
    loop = SpecDecodeLoop(m, cache, rows=2, max_len=48, draft_len=3, graph=False)
    with pytest.raises(ValueError, match="max_len=48"):
        loop.generate([[1], [2] * 37], 10)  # 37 + 10 - 1 + 3 = 49 keys
    with pytest.raises(ValueError, match="at least one token"):
        loop.generate([[1], []], 3)
    cache.add("other")
    cache.reserve("other", 33)  # three of the four blocks
    with pytest.raises(RuntimeError, match="cannot hold a prompt"):
        loop.generate([[1] * 3, [2] * 12], 4)  # the first runs and finishes; the second needs 12 + 3 + 3 = 18 keys, two blocks
    assert cache.free_blocks == 1 and (loop.remaining == 0).all() and (loop.pos == -1).all() and (loop.start == -1).all()
    passes = stub.passes
    for kw, exc, msg in ((dict(draft_len=0), ValueError, "draft_len"), (dict(draft_len=16), ValueError, "draft_len"),
                         (dict(ngram_max=0), ValueError, "ngram_max"), (dict(ngram_max=5), ValueError, "ngram_max"),
                         (dict(sync_every=8, u_stride=31), ValueError, "u_stride"), (dict(max_len=65), ValueError, "exceeds what the pool"),
                         (dict(max_len=3), ValueError, "must exceed draft_len"), (dict(rows=0), ValueError, "at least 1"),
                         (dict(rows=16384), ValueError, "65535 logits rows"), (dict(graph=True), RuntimeError, "graph=True needs the model on the GPU")):
        with pytest.raises(exc, match=msg):
            SpecDecodeLoop(m, cache, **dict(dict(rows=2, max_len=48, draft_len=3, graph=False), **kw))
    with pytest.raises(TypeError):
        SpecDecodeLoop(m, object(), rows=2, max_len=48, graph=False)
    m.model.unfuse_prefill()
    with pytest.raises(RuntimeError, match="fuse_prefill"):
        SpecDecodeLoop(m, cache, rows=2, max_len=48, graph=False)
    m.fuse_prefill()
    # generate(draft_len=...): refused before anything runs
    with pytest.raises(ValueError, match="device_loop=True"):
        m.generate([[1, 2]], 4, draft_len=3)
    with pytest.raises(ValueError, match="draft_len=-1"):
        m.generate([[1, 2]], 4, device_loop=True, draft_len=-1)
    with pytest.raises(ValueError, match="draft_len=16"):
        m.generate([[1, 2]], 4, device_loop=True, draft_len=16)
    assert stub.passes == passes and stub.prefills == [[3]] and cache.free_blocks == 1


def test_generate_draft_len_delegates_to_a_spec_loop(monkeypatch):
    m = _tiny_lm()
    made = []

    class _Loop:
        def __init__(self, lm, cache, rows, max_len, draft_len):
            made.append((lm, cache.num_blocks, rows, max_len, draft_len))

        def generate(self, *a):
            return ["delegated", a]

    monkeypatch.setattr("qqq_amd.serve.SpecDecodeLoop", _Loop)
    prompts = [[1, 2, 3], [4] * 20]
    got = m.generate(prompts, 9, 0.5, 7, 0.9, None, 3, device_loop=True, draft_len=5)
    assert got == ["delegated", (prompts, 9, 0.5, 7, 0.9, None, 3)]
    assert made == [(m, 1 + 3, 2, 48, 5)]  # budgets of 11 + 5 and 28 + 5 keys: 1 + 3 blocks, the longest rounded up to a block
