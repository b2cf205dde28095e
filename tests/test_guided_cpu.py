"""Guided decoding without a GPU: what the header declares, the two entries' argument checks (before any launch),
TokenFSM and its builders, tests/fsm_ref.py against TokenFSM on random automata, the kernels' code-object facts, the ops' refusals and fake
implementations, and generate_guided / GuidedDecodeLoop over the stub model of tests/test_step_cpu.py with fsm_ref standing in for the ops."""
import ctypes
import inspect
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch
from hypothesis import given, settings
from hypothesis import strategies as st

import fsm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qqq_amd_guided.h")
ERR_ARG = 17


@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


# ---- the header, the binding

def test_the_header_declares_the_two_entries_and_they_are_bound(L):
    from qqq_amd import _abi, _lib, build

    assert _lib.ABI_VERSION == 4 and L.qqq_amd_abi_version() == 4
    protos = _abi.prototypes(HEADER)
    assert set(protos) == {"qqq_fsm_mask", "qqq_fsm_advance"}
    assert len(protos["qqq_fsm_mask"][1]) == 14 and len(protos["qqq_fsm_advance"][1]) == 19
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert ret == "int" and fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), name
        assert all(p.rsplit(" ", 1)[0] in ("const void*", "void*", "int") for p in params), params
    unit = open(build.SRC).read()
    assert '#include "qqq_guided.hip.h"' in unit and '#include "../../include/qqq_amd_guided.h"' in unit


# fake device addresses with the alignment the entries ask for: the calls below must fail in the checks, before any launch
A8, A4, A2 = 0x20008, 0x30004, 0x40002
MASK = dict(logits=A2, state=A4, eos=A4, remaining=A4, offsets=A4, tokens=A4, accept=A4)
ADV = dict(out=A8, n_out=A4, n_fsm=A4, state=A4, eos=A4, offsets=A4, tokens=A4, next=A4, accept=A4, ids=A8, pos=A8, slots=A8, remaining=A4)


def _mask(L, ld=1008, n_states=5, n_edges=40, rows=6, vocab=1003, **ptrs):
    a = dict(MASK, **ptrs)
    return L.qqq_fsm_mask(a["logits"], ld, a["state"], a["eos"], a["remaining"], a["offsets"], a["tokens"], a["accept"], n_states, n_edges, rows,
                          vocab, 0, None)


def _adv(L, out_stride=40, n_states=5, n_edges=40, rows=6, **ptrs):
    a = dict(ADV, **ptrs)
    return L.qqq_fsm_advance(a["out"], out_stride, a["n_out"], a["n_fsm"], a["state"], a["eos"], a["offsets"], a["tokens"], a["next"], a["accept"],
                             n_states, n_edges, a["ids"], a["pos"], a["slots"], a["remaining"], rows, 0, None)


BAD_MASK = ([{name: None} for name in MASK if name not in ("eos", "remaining")] + [dict(logits=A2 + 1)]
            + [{name: A4 + 2} for name in MASK if MASK[name] == A4]
            + [dict(ld=1002), dict(ld=-1008), dict(vocab=0), dict(vocab=262145, ld=262152), dict(rows=-1), dict(rows=65536), dict(n_states=0),
               dict(n_states=-3), dict(n_edges=-1), dict(n_edges=0), dict(n_edges=0, tokens=None, vocab=-1)])
BAD_ADV = ([{name: None} for name in ADV if name != "eos"] + [{name: A8 + 4} for name in ("out", "ids", "pos", "slots")]
           + [{name: A4 + 2} for name in ADV if ADV[name] == A4]
           + [dict(out_stride=0), dict(out_stride=-40), dict(rows=-1), dict(rows=65536), dict(n_states=0), dict(n_edges=-1), dict(n_edges=0),
              dict(n_edges=0, tokens=None), dict(n_edges=0, next=None)])


@pytest.mark.parametrize("kw", BAD_MASK, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_fsm_mask_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _mask(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_fsm_mask:"), _lib.last_error()


@pytest.mark.parametrize("kw", BAD_ADV, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_fsm_advance_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _adv(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_fsm_advance:"), _lib.last_error()


def test_rows_0_is_a_no_op_with_null_pointers(L):
    z = None
    assert L.qqq_fsm_mask(z, 0, z, z, z, z, z, z, 0, 0, 0, 0, 0, z) == 0
    assert L.qqq_fsm_advance(z, 0, z, z, z, z, z, z, z, z, 0, 0, z, z, z, z, 0, 0, z) == 0
    assert _mask(L, rows=0) == 0 and _adv(L, rows=0) == 0


def test_guided_kernels_in_the_code_object_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB)}
    for name, lds in (("qqq_fsm_mask_kernel", 2048), ("qqq_fsm_advance_kernel", 0)):
        k = ks[name]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["max_flat_workgroup_size"] == 256 and k["group_segment_fixed_size"] == lds and k["vgpr_count"] <= 64, k


# ---- TokenFSM

def test_the_constructor_names_the_first_property_violated():
    from qqq_amd import TokenFSM

    good = dict(offsets=[0, 2, 3, 3], tokens=[1, 5, 2], next=[1, 2, 2], accept=[0, 0, 1], start=0, vocab=8)
    f = TokenFSM(**good)
    assert (f.n_states, f.n_edges, f.start) == (3, 3, 0) and f.offsets.dtype == f.tokens.dtype == f.next.dtype == f.accept.dtype == np.int32
    for bad, msg in ((dict(offsets=[[0, 2, 3, 3]]), "offsets must be a one-dimensional array of integers"),
                     (dict(tokens=[1.0, 5.0, 2.0]), "tokens must be a one-dimensional array of integers"),
                     (dict(next=[1, 2, 2 ** 31]), "next holds a value outside int32"),
                     (dict(accept=[], offsets=[0]), "accept must hold at least one state"),
                     (dict(offsets=[0, 2, 3]), r"offsets must hold S \+ 1 = 4 entries, not 3"),
                     (dict(offsets=[1, 2, 3, 3]), r"offsets\[0\] = 1 must be 0"),
                     (dict(offsets=[0, 3, 2, 3]), "offsets must be non-decreasing"),
                     (dict(offsets=[0, 2, 3, 4]), r"offsets\[S\] = 4 must be the number of edges E = 3"),
                     (dict(next=[1, 2]), "next must hold E = 3 entries like tokens, not 2"),
                     (dict(vocab=0), "vocab=0 must be at least 1"),
                     (dict(tokens=[1, 8, 2]), r"tokens holds an id outside \[0, 8\)"),
                     (dict(tokens=[-1, 5, 2]), r"tokens holds an id outside \[0, 8\)"),
                     (dict(tokens=[5, 5, 2]), "tokens must be strictly ascending inside each state"),
                     (dict(tokens=[5, 1, 2]), "tokens must be strictly ascending inside each state"),
                     (dict(next=[1, 3, 2]), r"next holds a state outside \[0, 3\)"),
                     (dict(next=[1, -1, 2]), r"next holds a state outside \[0, 3\)"),
                     (dict(start=3), r"start=3 outside \[0, 3\)"), (dict(start=-1), r"start=-1 outside \[0, 3\)")):
        with pytest.raises(ValueError, match="TokenFSM: " + msg):
            TokenFSM(**dict(good, **bad))
    assert TokenFSM([0, 2, 3, 3], [5, 7, 2], [1, 2, 2], [0, 0, 1]).vocab is None  # a descent across a state's border is none


def test_helpers_step_allowed_accepts_and_tensors():
    from qqq_amd import TokenFSM

    f = TokenFSM([0, 2, 3, 3], [1, 5, 2], [1, 2, 2], [0, 1, 0], 0, 8)
    assert f.allowed(0) == [1, 5] and f.allowed(1) == [2] and f.allowed(2) == [] and f.allowed(-1) == f.allowed(3) == []
    assert f.step(0, 1) == 1 and f.step(0, 5) == 2 and f.step(0, 2) == -2 and f.step(1, 2) == 2 and f.step(2, 1) == -2
    assert f.step(-1, 1) == -1 and f.step(-2, 1) == -2 and f.terminal(2) and not f.terminal(1) and not f.terminal(-1)
    assert f.accepts([5]) and f.accepts([1]) and f.accepts([1, 2]) and not f.accepts([]) and not f.accepts([2]) and not f.accepts([5, 1])
    assert f.accepts([1, 7], eos=7) and not f.accepts([1, 7]) and not f.accepts([7], eos=7) and not f.accepts([1, 7, 7], eos=7)
    assert f.walk([1, 7], eos=7) == 1 and f.walk([1, 7]) == -2 and f.walk([1, 2]) == 2
    t = f.tensors("cpu")
    assert t is f.tensors("cpu") and [x.dtype for x in t] == [torch.int32] * 4 and t[1].tolist() == [1, 5, 2] and t[3].tolist() == [0, 1, 0]


def test_from_choices_shares_prefixes_and_marks_inner_ends():
    from qqq_amd import TokenFSM

    f = TokenFSM.from_choices([[4, 5, 6], [4, 5], [4, 7], [9], [4, 5, 6]], vocab=50)  # a duplicate, a choice that is a prefix of another
    assert f.n_states == 6 and f.n_edges == 5 and f.start == 0 and f.allowed(0) == [4, 9]
    s45 = f.walk([4, 5])
    assert f.accept[s45] and f.allowed(s45) == [6] and not f.terminal(s45)
    for c in ([4, 5, 6], [4, 7], [9]):
        assert f.terminal(f.walk(c)) and f.accepts(c)
    assert f.accepts([4, 5]) and f.accepts([4, 5, 30], eos=30) and not f.accepts([4]) and not f.accepts([4, 30], eos=30) and not f.accepts([4, 5, 6, 6])
    with pytest.raises(ValueError, match="at least one choice"):
        TokenFSM.from_choices([])
    with pytest.raises(ValueError, match="tokens holds an id outside"):
        TokenFSM.from_choices([[50]], vocab=50)
    empty = TokenFSM.from_choices([[], [3]])
    assert empty.accept[0] and empty.accepts([]) and empty.accepts([3])


def test_from_allowed_is_one_accepting_state_of_self_loops():
    from qqq_amd import TokenFSM

    f = TokenFSM.from_allowed([7, 3, 3, 40], vocab=50)
    assert (f.n_states, f.n_edges) == (1, 3) and f.allowed(0) == [3, 7, 40] and f.next.tolist() == [0, 0, 0] and f.accept.tolist() == [1]
    assert f.accepts([3, 40, 7, 7]) and f.accepts([]) and f.accepts([3, 9], eos=9) and not f.accepts([3, 9])
    with pytest.raises(ValueError, match="at least one id"):
        TokenFSM.from_allowed([])


def test_merge_renumbers_and_gives_none_the_start_minus_one():
    from qqq_amd import TokenFSM

    a, b = TokenFSM.from_choices([[1, 2], [3]], vocab=9), TokenFSM.from_allowed([4, 5], vocab=7)
    m, starts = TokenFSM.merge([a, None, b, a])
    assert starts == [0, -1, a.n_states, 0] and m.n_states == a.n_states + 1 and m.n_edges == a.n_edges + 2 and m.vocab == 9
    assert m.allowed(starts[2]) == [4, 5] and m.step(starts[2], 4) == starts[2] and m.accept[starts[2]]
    for toks in ([1, 2], [3], [1], [4]):
        assert m.accepts(toks, start=starts[0]) == a.accepts(toks) and m.accepts(toks, start=starts[2]) == b.accepts(toks)
    one, starts = TokenFSM.merge([b, b])
    assert one is b and starts == [0, 0]
    none, starts = TokenFSM.merge([None, None])
    assert starts == [-1, -1] and none.n_states == 1 and none.n_edges == 0
    with pytest.raises(ValueError, match="TokenFSM or None"):
        TokenFSM.merge([a, "b"])


# [0-9]+(\.[0-9]+)? by hand: 0 -digit-> 1 -digit-> 1, 1 -'.'-> 2 -digit-> 3 -digit-> 3; finals 1 and 3.  State 4 is a trap the trim drops.
DIGITS = {ord(c) for c in "0123456789"}
DFA = {0: {**{d: 1 for d in DIGITS}, ord("x"): 4}, 1: {**{d: 1 for d in DIGITS}, ord("."): 2}, 2: {d: 3 for d in DIGITS},
       3: {d: 3 for d in DIGITS}, 4: {ord("x"): 4}}
VOCAB = [b"0", b"7", b"12", b".", b".5", b"3.", b"4.25", b"x", b"", b"a", b"1.2.", b"..", b"9x"]


def test_from_dfa_equals_the_regex_on_every_token_sequence_up_to_length_4():
    from qqq_amd import TokenFSM

    f = TokenFSM.from_dfa(DFA, 0, [1, 3], VOCAB)
    assert f.vocab == len(VOCAB)
    pattern = re.compile(rb"[0-9]+(\.[0-9]+)?")
    usable = [i for i, w in enumerate(VOCAB) if w]
    count = 0
    for n in range(0, 5):
        for seq in itertools.product(usable, repeat=n):
            text = b"".join(VOCAB[i] for i in seq)
            assert f.accepts(seq) == bool(pattern.fullmatch(text)), (seq, text)
            count += f.accepts(seq)
    assert count > 50
    # the trim: every kept state reaches a final one, none is a dead end, the empty token and the trap are nowhere
    for s in range(f.n_states):
        assert f.accept[s] or not f.terminal(s), s
        assert 8 not in f.allowed(s) and 7 not in f.allowed(s) and 12 not in f.allowed(s)
    reach = set(np.nonzero(f.accept)[0].tolist())
    for _ in range(f.n_states):
        reach |= {s for s in range(f.n_states) if any(f.step(s, t) in reach for t in f.allowed(s))}
    assert reach == set(range(f.n_states))
    with pytest.raises(ValueError, match="no sequence of tokens"):
        TokenFSM.from_dfa(DFA, 4, [1], VOCAB)


# ---- the reference against TokenFSM, on random automata

@st.composite
def _automata(draw):
    from qqq_amd import TokenFSM

    vocab = draw(st.integers(1, 40))
    S = draw(st.integers(1, 6))
    edges = [draw(st.dictionaries(st.integers(0, vocab - 1), st.integers(0, S - 1), max_size=min(vocab, 8))) for _ in range(S)]
    accept = draw(st.lists(st.integers(0, 1), min_size=S, max_size=S))
    return TokenFSM._from_edges(edges, accept, draw(st.integers(0, S - 1)), vocab)


@settings(max_examples=200, deadline=None, derandomize=True)
@given(_automata(), st.data())
def test_reference_mask_allows_exactly_allowed_and_advance_agrees_with_step(f, data):
    vocab, S = f.vocab, f.n_states
    eos = data.draw(st.integers(-1, vocab))
    states = np.array([data.draw(st.integers(-2, S)) for _ in range(4)], np.int32)
    rng = np.random.default_rng(data.draw(st.integers(0, 2 ** 16)))
    logits = rng.integers(0, 0x7C00, size=(4, vocab + 3)).astype(np.uint16)
    keep = logits.copy()
    fsm_ref.mask(logits, states, f.offsets, f.tokens, f.accept, eos=np.full(4, eos, np.int32), vocab=vocab)
    for r, s in enumerate(states.tolist()):
        if not 0 <= s < S:
            assert (logits[r] == keep[r]).all()
            continue
        allowed = set(f.allowed(s)) | ({eos} if f.accept[s] and 0 <= eos < vocab else set())
        assert set(np.nonzero(logits[r, :vocab] != 0xFC00)[0].tolist()) == allowed
        assert (logits[r, vocab:] == keep[r, vocab:]).all() and all(logits[r, v] == keep[r, v] for v in allowed)
    # a walk, one token per call, some of them outside the automaton
    n = data.draw(st.integers(1, 8))
    walk = [data.draw(st.integers(0, vocab - 1)) for _ in range(n)]
    out = np.array([walk], np.int64)
    z = lambda v, dt=np.int32: np.array([v], dt)  # noqa: E731
    state, n_fsm, ids, pos, slots, remaining = z(f.start), z(0), z(7, np.int64), z(5, np.int64), z(9, np.int64), z(3)
    s, retired = f.start, False
    for i, t in enumerate(walk):
        fsm_ref.advance(out, z(i + 1), n_fsm, state, f.offsets, f.tokens, f.next, f.accept, ids, pos, slots, remaining, eos=z(eos))
        if 0 <= s < S:
            to = f.step(s, t)
            stays = to == -2 and f.accept[s] and t == eos  # the eos in an accepting state: the sampler's business
            s = s if stays else to
            retired = retired or (not stays and (to == -2 or f.terminal(to)))  # a token outside, or a terminal state reached over an edge
        assert state[0] == s and n_fsm[0] == i + 1
        assert (remaining[0] == 0) == (ids[0] == 0) == (pos[0] == -1) == (slots[0] == -1) == retired
    assert state[0] == f.walk(walk, eos=eos)


def test_reference_advance_by_hand():
    # states: 0 -{1}-> 1 (accepting) -{2}-> 2 (terminal); 0 -{3}-> a next out of range
    offsets, tokens, nxt, accept = [0, 2, 3, 3], [1, 3, 2], [1, 9, 2], [0, 1, 0]
    out = np.array([[1, 2, 0], [1, 6, 0], [3, 0, 0], [1, 7, 0], [1, 2, 0], [1, 2, 0]], np.int64)
    n_out = np.array([2, 2, 1, 2, 1, 2], np.int32)
    n_fsm = np.array([0, 0, 0, 0, 1, 1], np.int32)  # row 0 two behind; row 4 has nothing new; row 5 one behind, from state 1
    state = np.array([0, 0, 0, 0, 1, 1], np.int32)
    ids, pos, slots, remaining = (np.full(6, v, dt) for v, dt in ((7, np.int64), (5, np.int64), (9, np.int64), (3, np.int32)))
    fsm_ref.advance(out, n_out, n_fsm, state, offsets, tokens, nxt, accept, ids, pos, slots, remaining, eos=np.full(6, 6, np.int32))
    assert state.tolist() == [2, 1, -2, -2, 1, 2] and n_fsm.tolist() == n_out.tolist()
    assert remaining.tolist() == [0, 3, 0, 0, 3, 0] and ids.tolist() == [0, 7, 0, 0, 7, 0] and pos.tolist() == [-1, 5, -1, -1, 5, -1]


# ---- the ops layer

def _tables(S=3, E=4):
    i32 = dict(dtype=torch.int32)
    return (torch.zeros(S + 1, **i32), torch.zeros(E, **i32), torch.zeros(E, **i32), torch.zeros(S, **i32))


def _mask_args(rows=3, vocab=40):
    return dict(logits=torch.zeros((rows, vocab), dtype=torch.float16), state=torch.zeros(rows, dtype=torch.int32), fsm_tensors=_tables(),
                eos=torch.zeros(rows, dtype=torch.int32), remaining=torch.zeros(rows, dtype=torch.int32))


def _adv_args(rows=3):
    i32, i64 = dict(dtype=torch.int32), dict(dtype=torch.int64)
    return dict(out=torch.zeros((rows, 9), **i64), n_out=torch.zeros(rows, **i32), n_fsm=torch.zeros(rows, **i32), state=torch.zeros(rows, **i32),
                fsm_tensors=_tables(), ids=torch.zeros(rows, **i64), pos=torch.zeros(rows, **i64), slots=torch.zeros(rows, **i64),
                remaining=torch.zeros(rows, **i32), eos=torch.zeros(rows, **i32))


def test_ops_are_exported_and_have_no_cpu_path():
    import qqq_amd
    from qqq_amd import ops

    assert qqq_amd.fsm_mask is ops.fsm_mask and qqq_amd.fsm_advance is ops.fsm_advance
    assert {"fsm_mask", "fsm_advance", "TokenFSM", "GuidedDecodeLoop"} <= set(qqq_amd.__all__)
    for args in (_mask_args(), dict(_mask_args(), eos=None, remaining=None)):
        with pytest.raises(RuntimeError, match="fsm_mask: .*no CPU path"):
            ops.fsm_mask(**args)
    for args in (_adv_args(), dict(_adv_args(), eos=None)):
        with pytest.raises(RuntimeError, match="fsm_advance: .*no CPU path"):
            ops.fsm_advance(**args)
    with pytest.raises(RuntimeError, match=r"fsm_mask: logits must be an fp16 \[rows, vocab\]"):
        ops.fsm_mask(**dict(_mask_args(), logits=torch.zeros(40, dtype=torch.float16)))
    with pytest.raises(RuntimeError, match=r"fsm_advance: out must be an int64 \[rows, out_stride\]"):
        ops.fsm_advance(**dict(_adv_args(), out=torch.zeros(9, dtype=torch.int64)))
    with pytest.raises(RuntimeError, match="fsm_mask: fsm_tensors must be the four tensors"):
        ops.fsm_mask(**dict(_mask_args(), fsm_tensors=_tables()[:3]))


def test_fake_implementations_check_dtypes_and_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from qqq_amd import ops

    i32 = dict(dtype=torch.int32)
    with FakeTensorMode():
        a = _mask_args()
        assert ops.fsm_mask(**a) is a["logits"] and ops.fsm_mask(**dict(a, eos=None, remaining=None)) is a["logits"]
        o, t, n, c = _tables()
        for bad, msg in ((dict(logits=torch.zeros((3, 40))), "logits must be fp16"), (dict(state=torch.zeros(3, dtype=torch.int64)), "state must be int32"),
                         (dict(state=torch.zeros(4, **i32)), "state must be int32"), (dict(eos=torch.zeros(2, **i32)), "eos must be int32"),
                         (dict(remaining=torch.zeros(3)), "remaining must be int32"),
                         (dict(fsm_tensors=(o.long(), t, n, c)), "offsets must be int32"), (dict(fsm_tensors=(o, t, n[:3], c)), "next must hold one entry per edge"),
                         (dict(fsm_tensors=(o[:3], t, n, c)), r"offsets S \+ 1 entries"),
                         (dict(logits=torch.zeros((40, 3), dtype=torch.float16).t()), "unit column stride")):
            with pytest.raises(RuntimeError, match="fsm_mask: .*" + msg):
                ops.fsm_mask(**dict(_mask_args(), **bad))
        assert ops.fsm_advance(**_adv_args()) is None and ops.fsm_advance(**dict(_adv_args(), eos=None)) is None
        for bad, msg in ((dict(out=torch.zeros((3, 9), **i32)), "out must be int64"), (dict(n_fsm=torch.zeros(4, **i32)), "n_fsm must be int32"),
                         (dict(ids=torch.zeros((3, 2), dtype=torch.int64)), "ids must be int64"), (dict(pos=torch.zeros(3, **i32)), "pos must be int64"),
                         (dict(slots=torch.zeros(2, dtype=torch.int64)), "slots must be int64"), (dict(remaining=torch.zeros(3, dtype=torch.int64)), "remaining must be int32"),
                         (dict(eos=torch.zeros(3, dtype=torch.int64)), "eos must be int32"), (dict(fsm_tensors=(o, t, n, c.float())), "accept must be int32")):
            with pytest.raises(RuntimeError, match="fsm_advance: .*" + msg):
                ops.fsm_advance(**dict(_adv_args(), **bad))


# ---- generate_guided and GuidedDecodeLoop over the stub model: fsm_ref stands in for the two ops

ORDER = ("ban_tokens", "fsm_mask", "sample_tokens", "sample_advance", "stop_check", "fsm_advance")


def _np(t):
    return None if t is None else t.numpy()


def _stub_mask(logits, state, fsm_tensors, eos=None, remaining=None):
    o, t, _, a = (x.numpy() for x in fsm_tensors)
    fsm_ref.mask(logits.numpy().view(np.uint16), state.numpy(), o, t, a, eos=_np(eos), remaining=_np(remaining))
    return logits


def _stub_advance(out, n_out, n_fsm, state, fsm_tensors, ids, pos, slots, remaining, eos=None):
    o, t, n, a = (x.numpy() for x in fsm_tensors)
    fsm_ref.advance(out.numpy(), n_out.numpy(), n_fsm.numpy(), state.numpy(), o, t, n, a, ids.numpy(), pos.numpy(), slots.numpy(),
                    remaining.numpy(), eos=_np(eos))


class _Guided:
    """generate_guided on the host path, or a GuidedDecodeLoop, over the stub model that continues t with t + 1 modulo 50; `calls` records
    the ops of ORDER as they are called"""

    def __init__(self, path, monkeypatch, rows=2, **loop_kw):
        import test_step_cpu as t
        from qqq_amd import GuidedDecodeLoop, ops
        from test_stop_cpu import _stub_ban, _stub_check

        self.m, self.path, self.calls = t._tiny_lm(), path, []
        self.stub = t._LoopStub(self.m, monkeypatch)
        monkeypatch.setattr(ops, "ban_tokens", _stub_ban([]))
        monkeypatch.setattr(ops, "stop_check", _stub_check([]))
        monkeypatch.setattr(ops, "fsm_mask", _stub_mask)
        monkeypatch.setattr(ops, "fsm_advance", _stub_advance)
        for name in ORDER:
            monkeypatch.setattr(ops, name, self._recorded(name, getattr(ops, name)))
        self.cache = self.m.new_cache(8, 16)
        self.loop = None
        if path == "loop":
            self.loop = GuidedDecodeLoop(self.m, self.cache, rows=rows, max_len=48, fsm_states=32, fsm_edges=64, sync_every=3, u_stride=4,
                                         graph=False, **loop_kw)

    def _recorded(self, name, f):
        def call(*a, **kw):
            self.calls.append(name)
            return f(*a, **kw)
        return call

    def __call__(self, prompts, fsm, new, **kw):
        if self.loop is None:
            return self.m.generate_guided(prompts, fsm, new, cache=self.cache, **kw)
        return self.loop.generate_guided(prompts, fsm, new, **kw)


def _up(first, n):
    return [(first + j) % 50 for j in range(n)]


@pytest.mark.parametrize("path", ["host", "loop"])
def test_guided_runs_over_host_stubs_counting_up(monkeypatch, path):
    from qqq_amd import TokenFSM

    g = _Guided(path, monkeypatch, **(dict(stops=True) if path == "loop" else {}))
    prompts = [[1, 2, 3], [10] * 17, [7], [20, 21]]  # more prompts than rows: rows are reused
    free = [_up(4, 9), _up(11, 9), _up(8, 9), _up(22, 9)]
    everything = TokenFSM.from_allowed(range(50), vocab=50)
    assert g(prompts, everything, 9) == free and g(prompts, None, 9) == free and g(prompts, [None] * 4, 9) == free
    # a choice the model would take ends at its terminal state without an eos; a masked successor is replaced by the lowest allowed id
    f0 = TokenFSM.from_choices([[4, 5, 6], [4, 7]], vocab=50)
    f1 = TokenFSM.from_choices([[11, 30, 31, 32]], vocab=50)
    f3 = TokenFSM.from_choices([[22], [23, 24]], vocab=50)  # its first token is already terminal: the row never starts
    got = g(prompts, [f0, f1, None, f3], 9)
    assert got == [[4, 5, 6], [11, 30, 31, 32], free[2], [22]]
    assert all(f is None or f.accepts(o) for f, o in zip([f0, f1, None, f3], got))
    # the end of a choice that another extends: the eos is drawable there, and nowhere else
    f = TokenFSM.from_choices([[4, 5], [4, 5, 9, 10]], vocab=50)
    assert g([[1, 2, 3]], f, 9, eos_token_id=6) == [[4, 5, 6]] and f.accepts([4, 5, 6], eos=6)
    assert g([[1, 2, 3]], f, 9, eos_token_id=5) == [[4, 5]]             # the eos is an explicit edge too: the edge is taken, the eos ends
    assert g([[1, 2, 3]], f, 9, eos_token_id=30) == [[4, 5, 9, 10]]     # 6 is masked, 9 the only edge
    assert g([[1, 2, 3]], f, 9, eos_token_id=6, min_new_tokens=3) == [[4, 5, 9, 10]]  # the ban goes first: the eos is -inf when the mask keeps it
    assert g([[1, 2, 3]], f, 3, eos_token_id=30) == [[4, 5, 9]]         # the budget ends it inside the automaton
    assert g([[1, 2, 3]], f, 9, stop=[[5, 9]]) == [[4]] and g([[1, 2, 3]], f, 9, stop_token_ids=[9]) == [[4, 5, 9]]
    assert g([[1, 2, 3]], f, 0) == [[]] and g([], f, 5) == []
    assert g.cache.free_blocks == 8
    if g.loop is not None:
        assert (g.loop.remaining == 0).all() and (g.loop.pos == -1).all() and g.loop.n_fsm.tolist() == g.loop.n_out.tolist()


@pytest.mark.parametrize("path", ["host", "loop"])
def test_the_mask_sits_between_ban_and_sampler_and_the_advance_behind_the_stop_check(monkeypatch, path):
    from qqq_amd import TokenFSM

    g = _Guided(path, monkeypatch, **(dict(stops=True) if path == "loop" else {}))
    f = TokenFSM.from_allowed(range(50), vocab=50)
    assert g([[1, 2, 3]], f, 5, eos_token_id=40, min_new_tokens=4, stop=[[45, 46]]) == [_up(4, 5)]
    first = g.calls[:3]
    assert first == ["ban_tokens", "fsm_mask", "sample_tokens"]  # the prefill's draw, on every path
    rest = g.calls[3:]
    if path == "host":  # the ban runs while a completion is below its minimum: three more passes, then the mask alone
        assert rest == ["ban_tokens", "fsm_mask", "sample_tokens"] * 3 + ["fsm_mask", "sample_tokens"]
    else:
        step = ["ban_tokens", "fsm_mask", "sample_advance", "stop_check", "fsm_advance"]
        assert len(rest) % 5 == 0 and rest == step * (len(rest) // 5) and len(rest) >= 20


def test_a_family_and_penalties_and_records_pass_through(monkeypatch):
    from qqq_amd import TokenFSM, ops
    from test_logprobs_cpu import _stub_topk, _stub_topk_step
    from test_penalty_cpu import _stub_penalize

    f = TokenFSM.from_choices([[4, 5, 9, 10], [8, 9, 12]], vocab=50)
    want = [[[4, 5, 9, 10]] * 2, [[8, 9, 12]] * 2]
    host = _Guided("host", monkeypatch)
    loop = _Guided("loop", monkeypatch, rows=2, family=2, logprobs=2, penalties=True, stops=True)
    monkeypatch.setattr(ops, "penalize_logits", _stub_penalize([]))
    monkeypatch.setattr(ops, "topk_logprobs", _stub_topk([]))
    monkeypatch.setattr(ops, "topk_logprobs_step", _stub_topk_step([]))
    toks, recs = host([[1, 2, 3], [7]], f, 9, n=2, logprobs=2, repetition_penalty=1.0001, min_new_tokens=2)
    toks_l, recs_l = loop([[1, 2, 3], [7]], f, 9, repetition_penalty=1.0001, min_new_tokens=2)
    assert toks == toks_l == want
    for fam, fam_l, fam_t in zip(recs, recs_l, want):
        for r, rl, t in zip(fam, fam_l, fam_t):
            assert r.top_ids[:, 0].tolist() == rl.top_ids[:, 0].tolist() == t  # the records show the masked row
    assert host.cache.free_blocks == 8 and loop.cache.free_blocks == 8 and (loop.loop.shared == 0).all()


def test_refusals(monkeypatch):
    from qqq_amd import GuidedDecodeLoop, TokenFSM

    g = _Guided("loop", monkeypatch)
    sig = inspect.signature(g.m.generate_guided).parameters
    assert list(sig)[:3] == ["prompts", "fsm", "max_new_tokens"] and list(sig)[-4:] == ["logprobs", "repetition_penalty", "presence_penalty", "frequency_penalty"]
    assert "draft_len" not in sig and "SpecDecodeLoop do not combine" in g.m.generate_guided.__doc__
    with pytest.raises(TypeError, match="draft_len"):
        g.m.generate_guided([[1, 2]], None, 3, draft_len=2)
    f = TokenFSM.from_allowed(range(50), vocab=50)
    for bad, msg in (([f], "fsm holds 1 entries for 2 prompts"), ([f, 3], "fsm must be a TokenFSM"), ("ab", "fsm must be a TokenFSM")):
        with pytest.raises(ValueError, match="generate_guided: " + msg):
            g.m.generate_guided([[1, 2], [3]], bad, 3, cache=g.cache)
        with pytest.raises(ValueError, match="GuidedDecodeLoop.generate_guided: " + msg):
            g.loop.generate_guided([[1, 2], [3]], bad, 3)
    with pytest.raises(ValueError, match="generate_guided: n=0"):
        g.m.generate_guided([[1, 2]], f, 3, n=0)
    with pytest.raises(ValueError, match="generate_guided: logprobs=33"):
        g.m.generate_guided([[1, 2]], f, 3, logprobs=33)
    # the capacities: an automaton beyond them raises before anything runs
    small = GuidedDecodeLoop(g.m, g.cache, rows=2, max_len=48, fsm_states=2, fsm_edges=40, graph=False)
    assert small.fsm_offsets.shape == (3,) and small.fsm_tokens.shape == small.fsm_next.shape == (40,) and small.fsm_accept.shape == (2,)
    assert small.fsm_state.tolist() == [-1, -1] and small.n_fsm.tolist() == [0, 0]
    passes = len(g.stub.free_seen)
    with pytest.raises(ValueError, match="3 states and 2 edges exceeds the loop's capacities fsm_states=2 and fsm_edges=40"):
        small.generate_guided([[1, 2, 3]], TokenFSM.from_choices([[4, 5]], vocab=50), 4)
    with pytest.raises(ValueError, match="1 states and 50 edges exceeds"):
        small.generate_guided([[1, 2, 3]], f, 4)
    assert len(g.stub.free_seen) == passes and g.cache.free_blocks == 8
    for kw in (dict(fsm_states=0), dict(fsm_edges=0)):
        with pytest.raises(ValueError, match="GuidedDecodeLoop: fsm_states"):
            GuidedDecodeLoop(g.m, g.cache, rows=2, max_len=48, graph=False, **kw)
    assert small.generate_guided([[1, 2, 3]], TokenFSM.from_choices([[4]], vocab=50), 4) == [[4]]
    assert small.generate([[1, 2, 3]], 4) == [_up(4, 4)]  # the plain call: no automaton


@pytest.mark.parametrize("path", ["host", "loop"])
def test_a_completion_that_leaves_its_automaton_raises_and_the_pool_is_left_as_found(monkeypatch, path):
    from qqq_amd import TokenFSM, ops

    g = _Guided(path, monkeypatch, **(dict(stops=True) if path == "loop" else {}))
    # below the minimum the only allowed token is the banned eos: every allowed logit is -inf, the argmax of such a row is token 0
    only = TokenFSM.from_choices([[4, 5], [4, 5, 6]], vocab=50)
    with pytest.raises(RuntimeError, match=r"generate(_guided)?: completion 0 .* drew a token outside its automaton"):
        g([[1, 2, 3], [7]], [TokenFSM.from_allowed([4], vocab=50), None], 6, eos_token_id=4, min_new_tokens=3)
    assert g.cache.free_blocks == 8
    assert g([[1, 2, 3]], only, 6) == [[4, 5, 6]]
    # an exception in the middle of a run
    count = [0]

    def boom(*a, **kw):
        count[0] += 1
        if count[0] >= 3:
            raise RuntimeError("boom")
        return (_stub_mask if path == "host" else _stub_advance)(*a, **kw)

    monkeypatch.setattr(ops, "fsm_mask" if path == "host" else "fsm_advance", boom)
    with pytest.raises(RuntimeError, match="boom"):
        g([[1, 2, 3], [0] * 17], TokenFSM.from_allowed(range(50), vocab=50), 12)
    assert count[0] == 3 and g.cache.free_blocks == 8
    if g.loop is not None:
        assert (g.loop.remaining == 0).all() and (g.loop.pos == -1).all() and (g.loop.fsm_state == -1).all()
        assert g.loop.n_fsm.tolist() == g.loop.n_out.tolist()


def test_device_loop_builds_a_guided_loop_with_capacities_rounded_up(monkeypatch):
    from qqq_amd import TokenFSM
    from test_step_cpu import _tiny_lm

    m = _tiny_lm()
    made = []

    class _Loop:
        def __init__(self, lm, cache, rows, max_len, **kw):
            made.append(kw)

        def generate_guided(self, *a, **kw):
            return ["delegated", a, kw]

    monkeypatch.setattr("qqq_amd.serve.GuidedDecodeLoop", _Loop)
    f = TokenFSM.from_choices([list(range(1, 41)), [3] * 30], vocab=50)  # 70 states, 69 edges
    args = ([[1, 2, 3], [4] * 20], 9, 0.5, 7, 0.9, None, 3)
    assert m.generate_guided(args[0], f, *args[1:], device_loop=True) == ["delegated", (args[0], f) + args[1:], {}]
    got = m.generate_guided(args[0], [f, None], *args[1:], device_loop=True, n=2, logprobs=1, min_new_tokens=2)
    assert got[2] == dict(stop=[], stop_token_ids=[], min_new_tokens=2)
    assert made == [dict(fsm_states=128, fsm_edges=128), dict(fsm_states=128, fsm_edges=128, family=2, logprobs=1, stops=True)]


def test_the_hooks_of_the_plain_paths_do_nothing(monkeypatch):
    """generate() and DecodeLoop call neither op; tests/test_generate_calls_cpu.py holds their recorded calls"""
    from qqq_amd import DecodeLoop

    g = _Guided("host", monkeypatch)
    loop = DecodeLoop(g.m, g.cache, rows=2, max_len=48, sync_every=3, u_stride=4, graph=False)
    assert g.m.generate([[1, 2, 3]], 5, cache=g.cache) == [_up(4, 5)] and loop.generate([[1, 2, 3]], 5) == [_up(4, 5)]
    assert "fsm_mask" not in g.calls and "fsm_advance" not in g.calls
    assert list(inspect.signature(DecodeLoop.__init__).parameters)[-1] == "stops"
