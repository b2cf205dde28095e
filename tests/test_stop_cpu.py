"""Stop sequences, stop token ids and min_new_tokens without a GPU: what the header declares, the two entries'
argument checks (before any launch), the ops' refusals and fake implementations, generate()'s three keywords and how they reach the
loops, and the bookkeeping of the host path, DecodeLoop and SpecDecodeLoop with host stubs for the forward pass, the samplers and --
through tests/stop_ref.py -- the two new ops."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import stop_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qqq_amd_stop.h")
ERR_ARG = 17


@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


# ---- the reference by hand

def _state(rows, group=1):
    z = lambda fill, dt=np.int32, shape=(rows,): np.full(shape, fill, dt)  # noqa: E731
    wide = (rows,) if group == 1 else (rows, group)
    return dict(n_seen=z(1), n_trim=z(0), stop_hit=z(-1), ids=z(7, np.int64, wide), pos=z(5, np.int64, wide), slots=z(9, np.int64, wide),
                remaining=z(3), min_new=z(0))


def test_reference_stop_check_by_hand():
    # the decode loop's addressing: the completion is first, then out
    out = np.array([[5, 6, 7, 8, 0, 0]] * 4, np.int64)
    st = _state(4)
    st["n_seen"][:] = [1, 1, 3, 4]
    n_out = np.array([3, 3, 3, 3], np.int32)  # completions [4, 5, 6, 7] each
    stop_ids = np.array([[6, 7, 0], [4, 5, 6], [5, 0, 0]], np.int32)
    stop_len = np.array([2, 3, 1], np.int32)
    stop_ref.stop_check(out, np.full(4, -1, np.int32), np.full(4, 4, np.int32), n_out, stop_ids, stop_len, **st)
    # row 0: e = 2 ends in [5] (sequence 2): trim 4 - 2 + 1; row 1 the same; row 2: e = 4 alone, [6, 7]; row 3: nothing new, untouched
    assert st["n_trim"].tolist() == [3, 3, 2, 0] and st["stop_hit"].tolist() == [2, 2, 0, -1]
    assert st["n_seen"].tolist() == [4, 4, 4, 4] and st["remaining"].tolist() == [0, 0, 0, 3] and st["pos"].tolist() == [-1, -1, -1, 5]
    # a minimum of 3 skips the end at 2: at e = 3 sequence 1 (which spans `first`) matches: everything goes
    st = _state(1)
    st["min_new"][:] = 3
    stop_ref.stop_check(out[:1], np.full(1, -1, np.int32), np.full(1, 4, np.int32), n_out[:1], stop_ids, stop_len, **st)
    assert st["n_trim"].tolist() == [4] and st["stop_hit"].tolist() == [1]
    # without `first` the same sequence finds no token at index -1; an end id keeps its token and goes before a sequence at the same end
    st = _state(1)
    stop_ref.stop_check(out[:1], np.full(1, -1, np.int32), None, n_out[:1], stop_ids[1:2], stop_len[1:2], **st, end_ids=[-1, 7])
    assert st["n_trim"].tolist() == [0] and st["stop_hit"].tolist() == [1 + 1] and st["ids"].tolist() == [0]
    # the row's eos goes before the end ids and before a sequence that ends in it, at any length -- also below the minimum
    for least in (0, 9):
        st = _state(1)
        st["min_new"][:] = least
        stop_ref.stop_check(out[:1], np.full(1, -1, np.int32), np.full(1, 4, np.int32), n_out[:1], np.array([[5, 6], [6, 0]], np.int32),
                            np.array([2, 1], np.int32), **st, end_ids=[6], eos=np.array([6], np.int32))
        assert st["n_trim"].tolist() == [1] and st["stop_hit"].tolist() == [2 + 1] and st["remaining"].tolist() == [0]
    st = _state(1)
    stop_ref.stop_check(out[:1], np.full(1, -1, np.int32), np.full(1, 4, np.int32), n_out[:1], np.array([[5, 6]], np.int32),
                        np.array([2], np.int32), **st, eos=np.array([-1], np.int32))
    assert st["n_trim"].tolist() == [3] and st["stop_hit"].tolist() == [0]
    # the speculative loop's addressing: the completion follows the prompt in hist; G entries retire
    hist = np.array([[9, 9, 4, 5, 6, 7, 8, 0]], np.int32)
    st = _state(1, group=3)
    start = np.array([6], np.int64)
    stop_ref.stop_check(hist, np.array([2], np.int32), None, np.array([4], np.int32), stop_ids[:1], stop_len[:1], **st, start=start)
    assert st["n_trim"].tolist() == [3] and st["ids"].tolist() == [[0] * 3] and st["slots"].tolist() == [[-1] * 3] and start.tolist() == [-1]


def test_reference_ban_tokens_by_hand():
    logits = np.arange(2 * 2 * 8, dtype=np.float16).reshape(4, 8)
    keep = logits.copy()
    stop_ref.ban_tokens(logits, np.array([1, 2], np.int32), np.array([3, 3], np.int32), np.array([0, -1], np.int32), [5, 9, -1, 5], base=0,
                        vocab=6)
    # row 0: indices 1 and 2 are below 3; row 1: index 2 alone
    want = keep.copy()
    want[0, [0, 5]] = want[1, [0, 5]] = -np.inf
    want[2, 5] = -np.inf
    assert np.array_equal(logits.view(np.uint16), want.view(np.uint16))


# ---- the C ABI

def test_the_header_declares_the_two_entries(L):
    from qqq_amd import _abi, _lib, build

    assert _lib.ABI_VERSION == 4 and L.qqq_amd_abi_version() == 4
    protos = _abi.prototypes(HEADER)
    assert set(protos) == {"qqq_ban_tokens", "qqq_stop_check"}
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert ret == "int" and fn.restype is __import__("ctypes").c_int and len(fn.argtypes) == len(params), name
        assert all(p.rsplit(" ", 1)[0] in ("const void*", "void*", "int") for p in params), params
    unit = open(build.SRC).read()
    assert '#include "qqq_stop.hip.h"' in unit and '#include "../../include/qqq_amd_stop.h"' in unit


# fake device addresses with the alignment the entries ask for: the calls below must fail in the checks, before any launch
A8, A4, A2 = 0x20008, 0x30004, 0x40002
BAN = dict(logits=A2, n_out=A4, min_new=A4, eos=A4, ban_ids=A4)
CHECK = dict(tokens=A8, base=A4, first=A4, n_out=A4, stop_ids=A4, stop_len=A4, end_ids=A4, eos=A4, min_new=A4, n_seen=A4, n_trim=A4, stop_hit=A4,
             ids=A8, pos=A8, slots=A8, start=A8, remaining=A4)


def _ban(L, ld=1008, base=1, n_ban=4, group=3, rows=6, vocab=1003, **ptrs):
    a = dict(BAN, **ptrs)
    return L.qqq_ban_tokens(a["logits"], ld, a["n_out"], base, a["min_new"], a["eos"], a["ban_ids"], n_ban, group, rows, vocab, 0, None)


def _check(L, token_bytes=8, tok_stride=40, stop_stride=32, n_stop=32, n_end=32, group=3, rows=6, **ptrs):
    a = dict(CHECK, **ptrs)
    return L.qqq_stop_check(a["tokens"], token_bytes, tok_stride, a["base"], a["first"], a["n_out"], a["stop_ids"], stop_stride,
                            a["stop_len"], n_stop, a["end_ids"], n_end, a["eos"], a["min_new"], a["n_seen"], a["n_trim"], a["stop_hit"], a["ids"],
                            a["pos"], a["slots"], a["start"], a["remaining"], group, rows, 0, None)


BAD_BAN = ([{name: None} for name in BAN] + [dict(logits=A2 + 1)] + [{name: A4 + 2} for name in ("n_out", "min_new", "eos", "ban_ids")]
           + [dict(group=g) for g in (0, 17, -1)] + [dict(n_ban=33), dict(n_ban=-1), dict(n_ban=0), dict(ld=1002), dict(ld=-1008),
                                                     dict(vocab=0), dict(vocab=262145, ld=262152), dict(rows=-1), dict(rows=65536),
                                                     dict(rows=30000, group=3)])
BAD_CHECK = ([{name: None} for name in CHECK if name not in ("first", "eos", "start")] + [dict(tokens=A8 + 4), dict(tokens=A4 + 2, token_bytes=4)]
             + [{name: A8 + 4} for name in ("ids", "pos", "slots", "start")]
             + [{name: A4 + 2} for name in CHECK if CHECK[name] == A4]
             + [dict(group=g) for g in (0, 17, -1)] + [dict(token_bytes=b) for b in (0, 2, 16, -4)]
             + [dict(n_stop=33), dict(n_stop=-1), dict(stop_stride=33), dict(stop_stride=0), dict(stop_stride=-32), dict(n_end=33),
                dict(n_end=-1), dict(tok_stride=0), dict(tok_stride=-40), dict(n_stop=0), dict(n_end=0), dict(rows=-1), dict(rows=65536)])


@pytest.mark.parametrize("kw", BAD_BAN, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_ban_tokens_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _ban(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_ban_tokens:"), _lib.last_error()


@pytest.mark.parametrize("kw", BAD_CHECK, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_stop_check_rejects_bad_arguments(L, kw):
    from qqq_amd import _lib

    assert _check(L, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_stop_check:"), _lib.last_error()


def test_rows_0_is_a_no_op_with_null_pointers(L):
    z = None
    assert L.qqq_ban_tokens(z, 0, z, 0, z, z, z, 0, 0, 0, 0, 0, z) == 0
    assert L.qqq_stop_check(z, 0, 0, z, z, z, z, 0, z, 0, z, 0, z, z, z, z, z, z, z, z, z, z, 0, 0, 0, z) == 0
    assert _ban(L, rows=0) == 0 and _check(L, rows=0) == 0


def test_stop_kernels_in_the_code_object_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    build.build()
    ks = {k["demangled"]: k for k in code_object.kernels(build.LIB)}
    for name in ("qqq_ban_tokens_kernel", "qqq_stop_check_kernel"):
        k = ks[name]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["max_flat_workgroup_size"] == 256 and k["group_segment_fixed_size"] == 0 and k["vgpr_count"] <= 64, k


# ---- the ops layer

def _ban_args(rows=3, g=2, vocab=40):
    i32 = dict(dtype=torch.int32)
    return dict(logits=torch.zeros((rows * g, vocab), dtype=torch.float16), n_out=torch.zeros(rows, **i32), min_new=torch.zeros(rows, **i32),
                eos=torch.zeros(rows, **i32), ban_ids=torch.zeros(4, **i32), base=1)


def _check_args(rows=3, g=2, dtype=torch.int64, start=True):
    i32, i64 = dict(dtype=torch.int32), dict(dtype=torch.int64)
    row = lambda: torch.zeros(rows, **i32)  # noqa: E731
    return dict(tokens=torch.zeros((rows, 9), dtype=dtype), base=row(), first=row(), n_out=row(), stop_ids=torch.zeros((32, 32), **i32),
                stop_len=torch.zeros(32, **i32), min_new=row(), n_seen=row(), n_trim=row(), stop_hit=row(), ids=torch.zeros((rows, g), **i64),
                pos=torch.zeros((rows, g), **i64), slots=torch.zeros((rows, g), **i64), remaining=row(),
                start=torch.zeros(rows, **i64) if start else None, end_ids=torch.zeros(32, **i32), eos=row())


def test_ops_are_exported_and_have_no_cpu_path():
    import qqq_amd
    from qqq_amd import ops

    assert qqq_amd.ban_tokens is ops.ban_tokens and qqq_amd.stop_check is ops.stop_check
    assert {"ban_tokens", "stop_check"} <= set(qqq_amd.__all__)
    with pytest.raises(RuntimeError, match="ban_tokens: .*no CPU path"):
        ops.ban_tokens(**_ban_args())
    with pytest.raises(RuntimeError, match="ban_tokens: .*no CPU path"):
        ops.ban_tokens(**dict(_ban_args(), ban_ids=None))
    with pytest.raises(RuntimeError, match="stop_check: .*no CPU path"):
        ops.stop_check(**_check_args())
    with pytest.raises(RuntimeError, match="stop_check: .*no CPU path"):
        ops.stop_check(**dict(_check_args(dtype=torch.int32, start=False), first=None, end_ids=None))
    with pytest.raises(RuntimeError, match=r"fp16 \[rows \* group, vocab\]"):
        ops.ban_tokens(**dict(_ban_args(), logits=torch.zeros(40, dtype=torch.float16)))
    with pytest.raises(RuntimeError, match=r"int32 or int64 \[rows, stride\]"):
        ops.stop_check(**dict(_check_args(), tokens=torch.zeros(9, dtype=torch.int64)))


def test_fake_implementations_check_dtypes_and_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from qqq_amd import ops

    with FakeTensorMode():
        a = _ban_args()
        assert ops.ban_tokens(**a) is a["logits"] and ops.ban_tokens(**dict(a, ban_ids=None)) is a["logits"]
        for bad, msg in ((dict(logits=torch.zeros((6, 40))), "logits must be fp16"), (dict(n_out=torch.zeros(3, dtype=torch.int64)), "n_out must be int32"),
                         (dict(n_out=torch.zeros(4, dtype=torch.int32)), "logits hold 6 rows"), (dict(eos=torch.zeros(2, dtype=torch.int32)), "eos must be int32"),
                         (dict(min_new=torch.zeros(3)), "min_new must be int32"), (dict(ban_ids=torch.zeros(33, dtype=torch.int32)), "ban_ids must be int32"),
                         (dict(logits=torch.zeros((40, 6), dtype=torch.float16).t()), "unit column stride")):
            with pytest.raises(RuntimeError, match=msg):
                ops.ban_tokens(**dict(_ban_args(), **bad))
        with pytest.raises(RuntimeError, match="1 <= group <= 16"):
            ops.ban_tokens(**dict(_ban_args(), logits=torch.zeros((3 * 17, 40), dtype=torch.float16)))
        assert ops.stop_check(**_check_args()) is None
        assert ops.stop_check(**dict(_check_args(dtype=torch.int32, g=1, start=False), first=None, end_ids=None)) is None
        one = _check_args()
        assert ops.stop_check(**dict(one, ids=one["ids"][:, 0].contiguous(), pos=one["pos"][:, 0].contiguous(),
                                     slots=one["slots"][:, 0].contiguous())) is None
        i32 = dict(dtype=torch.int32)
        for bad, msg in ((dict(tokens=torch.zeros((3, 9), dtype=torch.int16)), "tokens must be int32 or int64"),
                         (dict(ids=torch.zeros((3, 17), dtype=torch.int64)), "ids must be int64"), (dict(pos=torch.zeros((3, 3), dtype=torch.int64)), "pos must be int64"),
                         (dict(slots=torch.zeros((3, 2), **i32)), "slots must be int64"), (dict(start=torch.zeros(3, **i32)), "start must be int64"),
                         (dict(n_seen=torch.zeros(4, **i32)), "n_seen must be int32"), (dict(first=torch.zeros(3, dtype=torch.int64)), "first must be int32"),
                         (dict(stop_ids=torch.zeros((33, 32), **i32)), "stop_ids must be int32"), (dict(stop_ids=torch.zeros((32, 33), **i32)), "stop_ids must be int32"),
                         (dict(stop_len=torch.zeros(31, **i32)), "stop_len must be int32"), (dict(eos=torch.zeros(3, dtype=torch.int64)), "eos must be int32"), (dict(end_ids=torch.zeros(33, **i32)), "end_ids must be int32")):
            with pytest.raises(RuntimeError, match=msg):
                ops.stop_check(**dict(_check_args(), **bad))


# ---- generate(): the keywords

def test_the_keywords_stand_between_device_loop_and_n_and_are_checked():
    from qqq_amd import DecodeLoop, SpecDecodeLoop
    from test_step_cpu import _tiny_lm

    m = _tiny_lm()
    sig = inspect.signature(m.generate).parameters
    names = list(sig)
    at = names.index("device_loop")
    assert names[at + 1:at + 5] == ["stop", "stop_token_ids", "min_new_tokens", "n"]
    assert sig["stop"].default is None and sig["stop_token_ids"].default is None and sig["min_new_tokens"].default == 0
    for loop in (DecodeLoop, SpecDecodeLoop):
        assert list(inspect.signature(loop.__init__).parameters)[-1] == "stops" and inspect.signature(loop.__init__).parameters["stops"].default is False
        assert list(inspect.signature(loop.generate).parameters)[-4:] == ["frequency_penalty", "stop", "stop_token_ids", "min_new_tokens"]
    for kw, arg in ((dict(stop=[[1]] * 33), "stop"), (dict(stop=[[]]), "stop"), (dict(stop=[[1] * 33]), "stop"), (dict(stop=[[50]]), "stop"),
                    (dict(stop=[[-1]]), "stop"), (dict(stop=[1, 2]), "stop"), (dict(stop="ab"), "stop"), (dict(stop=[[1.5]]), "stop"),
                    (dict(stop_token_ids=[50]), "stop_token_ids"), (dict(stop_token_ids=list(range(33))), "stop_token_ids"),
                    (dict(stop_token_ids=3), "stop_token_ids"), (dict(min_new_tokens=-1), "min_new_tokens"), (dict(min_new_tokens=1.5), "min_new_tokens"),
                    (dict(stop=np.array([1, 2])), "stop"), (dict(stop=[np.int64(3)]), "stop"), (dict(stop=[[True]]), "stop"), (dict(stop=7), "stop"),
                    (dict(stop_token_ids=np.array([50])), "stop_token_ids"), (dict(stop_token_ids=[True]), "stop_token_ids"),
                    (dict(stop_token_ids="7"), "stop_token_ids"), (dict(min_new_tokens=True), "min_new_tokens")):
        for extra in (dict(), dict(device_loop=True)):
            with pytest.raises(ValueError, match=f"generate: {arg}"):
                m.generate([[1, 2]], 3, **kw, **extra)


def test_generate_passes_the_keywords_on_only_when_one_is_set(monkeypatch):
    from qqq_amd.model import stop_arguments
    from test_step_cpu import _tiny_lm

    # arrays, tensors and numpy integers are taken like lists and ints
    assert stop_arguments("f", 50, np.array([[1, 2], [3, 4]]), torch.tensor([5]), np.int64(2)) == ([[1, 2], [3, 4]], [5], 2)
    assert stop_arguments("f", 50, None, None, 0) == stop_arguments("f", 50, [], (), 0) == ([], [], 0)
    m = _tiny_lm()
    made = []

    class _Loop:
        def __init__(self, lm, cache, rows, max_len, *a, **kw):
            made.append((a, kw))

        def generate(self, *a, **kw):
            return ["delegated", a, kw]

    monkeypatch.setattr("qqq_amd.serve.DecodeLoop", _Loop)
    monkeypatch.setattr("qqq_amd.serve.SpecDecodeLoop", _Loop)
    args = ([[1, 2, 3], [4] * 20], 9, 0.5, 7, 0.9, None, 3)
    assert m.generate(*args, device_loop=True) == ["delegated", args, {}]  # as today
    assert m.generate(*args, device_loop=True, stop=None, stop_token_ids=None, min_new_tokens=0) == ["delegated", args, {}]
    assert m.generate(*args, device_loop=True, stop=[], stop_token_ids=(), draft_len=2) == ["delegated", args, {}]
    assert made == [((), {}), ((), {}), ((), dict(draft_len=2))]
    del made[:]
    off = dict(stop=[], stop_token_ids=[], min_new_tokens=0)
    assert m.generate(*args, device_loop=True, stop=[(7, 8)]) == ["delegated", args, dict(off, stop=[[7, 8]])]
    assert m.generate(*args, device_loop=True, stop_token_ids=(9,), draft_len=2) == ["delegated", args, dict(off, stop_token_ids=[9])]
    got = m.generate(*args, device_loop=True, min_new_tokens=4, n=2, logprobs=1, presence_penalty=0.5)
    assert got[1] == args and got[2] == dict(off, min_new_tokens=4, repetition_penalty=1.0, presence_penalty=0.5, frequency_penalty=0.0)
    assert made == [((), dict(stops=True)), ((), dict(draft_len=2, stops=True)), ((), dict(family=2, penalties=True, logprobs=1, stops=True))]


# ---- the bookkeeping of the three paths, with host stubs: the reference stands in for the two ops

def _np(t):
    return None if t is None else t.numpy()


def _stub_ban(calls):
    def ban_tokens(logits, n_out, min_new, eos, ban_ids=None, base=0):
        calls.append((logits.shape[0], n_out.shape[0], base))
        stop_ref.ban_tokens(logits.numpy(), n_out.numpy(), min_new.numpy(), eos.numpy(), [] if ban_ids is None else ban_ids.tolist(), base)
        return logits

    return ban_tokens


def _stub_check(calls):
    def stop_check(tokens, base, first, n_out, stop_ids, stop_len, min_new, n_seen, n_trim, stop_hit, ids, pos, slots, remaining, start=None,
                   end_ids=None, eos=None):
        calls.append(tokens.dtype)
        stop_ref.stop_check(tokens.numpy(), base.numpy(), _np(first), n_out.numpy(), stop_ids.numpy(), stop_len.numpy(), min_new.numpy(),
                            n_seen.numpy(), n_trim.numpy(), stop_hit.numpy(), ids.numpy(), pos.numpy(), slots.numpy(), remaining.numpy(),
                            start=_np(start), end_ids=[] if end_ids is None else end_ids.tolist(), eos=_np(eos))

    return stop_check


class _Paths:
    """generate() of the host path, a DecodeLoop and a SpecDecodeLoop over one stub model that counts up modulo `mod`, all with stubs"""

    def __init__(self, path, monkeypatch, rows=2, **loop_kw):
        from qqq_amd import DecodeLoop, SpecDecodeLoop

        if path == "spec":
            import test_spec_cpu as t

            self.m, self.mod = t._tiny_lm(), t.MOD
        else:
            import test_step_cpu as t

            self.m, self.mod = t._tiny_lm(), 50
        self.path, self.stub, self.bans, self.checks = path, t._LoopStub(self.m, monkeypatch), [], []
        monkeypatch.setattr("qqq_amd.model.ops.sample_tokens", lambda logits, T, k, p, u: logits.argmax(dim=1))
        for mod in ("model", "serve"):
            monkeypatch.setattr(f"qqq_amd.{mod}.ops.ban_tokens", _stub_ban(self.bans))
        monkeypatch.setattr("qqq_amd.serve.ops.stop_check", _stub_check(self.checks))
        self.cache = self.m.new_cache(8, 16)
        self.loop = None
        if path == "decode":
            self.loop = DecodeLoop(self.m, self.cache, rows=rows, max_len=48, sync_every=3, u_stride=4, graph=False, stops=True, **loop_kw)
        elif path == "spec":
            self.loop = SpecDecodeLoop(self.m, self.cache, rows=rows, max_len=48, draft_len=3, sync_every=3, graph=False, stops=True, **loop_kw)

    def up(self, first, n):
        return [(first + j) % self.mod for j in range(n)]

    def __call__(self, prompts, new, **kw):
        if self.loop is None:
            return self.m.generate(prompts, new, cache=self.cache, **kw)
        return self.loop.generate(prompts, new, **kw)


@pytest.mark.parametrize("path", ["host", "decode"])
def test_stops_over_host_stubs_counting_up(monkeypatch, path):
    """the stub model continues t with t + 1: the prompt [1, 2, 3] runs 4, 5, 6, ...; a banned successor leaves a row of zeros and -inf,
    whose argmax is token 0"""
    g = _Paths(path, monkeypatch)
    free = [g.up(4, 9), g.up(11, 9), g.up(8, 9), g.up(22, 9)]
    prompts = [[1, 2, 3], [10] * 17, [7], [20, 21]]  # more prompts than rows: rows are reused
    first_bans = lambda: [b for b in g.bans if b[2] == 0]  # noqa: E731  (the host's own: a loop's step bans with base 1 in every pass)
    assert g(prompts, 9) == free and first_bans() == []
    assert g(prompts, 9, stop=[[7, 8]]) == [[4, 5, 6], free[1], free[2], free[3]]  # cut in front of the match; the 8 of prompt 2 is a first token
    assert g(prompts, 9, stop=[[30], [7, 8], [14, 15, 16]]) == [[4, 5, 6], [11, 12, 13], g.up(8, 6), g.up(22, 8)]
    assert g(prompts, 9, stop=[[4, 5]]) == [[], free[1], free[2], free[3]]            # a match that includes the first token
    assert g(prompts, 9, stop=[[4], [22]]) == [[], free[1], free[2], []]              # a length-1 stop on the first token
    assert g(prompts, 9, stop=[[7]]) == [[4, 5, 6], free[1], free[2], free[3]]        # the prompt [7] is never matched
    assert g(prompts, 9, stop_token_ids=[6, 11]) == [[4, 5, 6], [11], [8, 9, 10, 11], free[3]]  # a stop id stays
    assert g(prompts, 9, stop_token_ids=[6], stop=[[6], [5, 6]]) == [[4, 5, 6], free[1], free[2], free[3]]  # ... and goes before a sequence
    assert first_bans() == []  # no minimum: the host never bans
    # min_new_tokens defers eos: 6 is banned at index 2, the row's argmax is 0, and the run goes on to the next 6
    assert g([[1, 2, 3]], 12, eos_token_id=6, min_new_tokens=5) == [[4, 5, 0, 1, 2, 3, 4, 5, 6]] and first_bans()
    assert g([[1, 2, 3]], 12, stop_token_ids=[6], min_new_tokens=3) == [[4, 5, 0, 1, 2, 3, 4, 5, 6]]
    assert g([[1, 2, 3]], 12, eos_token_id=6, min_new_tokens=2) == [[4, 5, 6]]
    # ... and skips the ends below it: [5] ends at length 2 alone, [5, 6] at length 3 -- and its cut leaves fewer than the minimum
    assert g([[1, 2, 3]], 9, stop=[[5]], min_new_tokens=3) == [free[0]]
    assert g([[1, 2, 3]], 9, stop=[[5, 6]], min_new_tokens=3) == [[4]]
    assert g([[1, 2, 3]], 9, stop=[[4]], min_new_tokens=1) == [[]] and g([[1, 2, 3]], 9, stop=[[4]], min_new_tokens=2) == [free[0]]
    # the budget wins over the minimum
    assert g([[1, 2, 3], [7]], 4, eos_token_id=5, min_new_tokens=20) == [[4, 0, 1, 2], [8, 9, 10, 11]]
    assert g([[1, 2, 3]], 1, stop=[[4]]) == [[]] and g([[1, 2, 3]], 0, stop=[[4]]) == [[]]
    assert g.cache.free_blocks == 8
    if path == "decode":
        assert g.checks and all(d == torch.int64 for d in g.checks)
        assert g.loop.n_seen.tolist() == (g.loop.n_out + 1).tolist() and (g.loop.remaining == 0).all() and (g.loop.pos == -1).all()


def test_spec_loop_stops_over_host_stubs_equal_the_host_path(monkeypatch):
    """the stub model counts up modulo 5, a period the drafter finds: steps emit several tokens and a match falls inside a step"""
    g = _Paths("spec", monkeypatch)
    prompts = [[1, 2, 3], [0] * 17, [4], [3, 4]]
    free = [g.up(4, 9), g.up(1, 9), g.up(0, 9), g.up(0, 9)]
    assert g(prompts, 9) == free
    assert g(prompts, 9, stop=[[2, 3]]) == [[4, 0, 1], [1], [0, 1], [0, 1]]
    assert g(prompts, 9, stop=[[4, 0]]) == [[], [1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3]]
    assert g(prompts, 9, stop=[[4]]) == [[], [1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3]]
    assert g(prompts, 9, stop_token_ids=[3]) == [[4, 0, 1, 2, 3], [1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3]]
    assert g.loop.accepted > 0 and all(d == torch.int32 for d in g.checks)
    host = _Paths("spec", monkeypatch)
    host.loop = None
    for kw in (dict(stop=[[2, 3, 4], [0, 1, 2, 3]], min_new_tokens=6), dict(eos_token_id=1, min_new_tokens=5), dict(stop_token_ids=[2, 4], min_new_tokens=3),
               dict(stop=[[1]], min_new_tokens=4, stop_token_ids=[0]), dict(eos_token_id=0, min_new_tokens=30)):
        want = host(prompts, 12, **kw)
        assert g(prompts, 12, **kw) == want, kw
        assert all(len(w) <= 12 for w in want)
    assert g([[1, 2, 3]], 12, eos_token_id=1, min_new_tokens=5) == [[4, 0, 0, 0, 0, 1]]
    assert g.cache.free_blocks == 8 and (g.loop.remaining == 0).all() and (g.loop.start == -1).all()


@pytest.mark.parametrize("path", ["host", "decode"])
def test_records_are_cut_like_their_tokens(monkeypatch, path):
    from test_logprobs_cpu import _stub_topk, _stub_topk_step

    g = _Paths(path, monkeypatch, **(dict(logprobs=2) if path == "decode" else {}))
    for mod in ("model", "serve"):
        monkeypatch.setattr(f"qqq_amd.{mod}.ops.topk_logprobs", _stub_topk([]))
    monkeypatch.setattr("qqq_amd.serve.ops.topk_logprobs_step", _stub_topk_step([]))
    kw = dict(logprobs=2) if path == "host" else {}
    toks, recs = g([[1, 2, 3], [10] * 17, [7]], 9, stop=[[7, 8], [11]], stop_token_ids=[10], **kw)
    assert toks == [[4, 5, 6], [], [8, 9, 10]]
    for t, r in zip(toks, recs):
        assert r.logprob.shape == r.rank.shape == (len(t),) and r.top_ids.shape == r.top_logprobs.shape == (len(t), 2)
        assert r.top_ids[:, 0].tolist() == t
    # the banned row is the one the records are taken from: the deferred eos has log-probability -inf there
    toks, recs = g([[1, 2, 3]], 12, eos_token_id=6, min_new_tokens=5, **kw)
    assert toks == [[4, 5, 0, 1, 2, 3, 4, 5, 6]] and recs[0].top_ids[:, 0].tolist() == toks[0] and 6 not in recs[0].top_ids[2].tolist()


@pytest.mark.parametrize("path", ["decode", "spec"])
def test_a_loop_without_the_flag_refuses_the_keywords_and_owns_nothing(monkeypatch, path):
    from qqq_amd import DecodeLoop, SpecDecodeLoop

    g = _Paths(path, monkeypatch)
    plain = (DecodeLoop(g.m, g.cache, rows=2, max_len=48, sync_every=3, u_stride=4, graph=False) if path == "decode" else
             SpecDecodeLoop(g.m, g.cache, rows=2, max_len=48, draft_len=3, sync_every=3, graph=False))
    names = ("min_new", "n_seen", "n_trim", "stop_hit", "stop_base", "first", "stop_ids", "stop_len", "ban_ids")
    assert not plain.stops and not any(hasattr(plain, a) for a in names)
    assert g.loop.stops and all(hasattr(g.loop, a) for a in names if a != "first") and hasattr(g.loop, "first") == (path == "decode")
    assert g.loop.stop_ids.shape == (32, 32) and g.loop.stop_len.shape == g.loop.ban_ids.shape == (32,)
    for kw in (dict(stop=[[1]]), dict(stop_token_ids=[1]), dict(min_new_tokens=2)):
        with pytest.raises(ValueError, match="need a loop built with stops=True"):
            plain.generate([[1, 2, 3]], 5, **kw)
    assert plain.generate([[1, 2, 3]], 5, stop=[], stop_token_ids=None) == [g.up(4, 5)] and g.checks == [] and g.cache.free_blocks == 8
    # the flagged loop without keywords: the ops ride along, the tokens are the plain loop's
    assert g.loop.generate([[1, 2, 3]], 5) == [g.up(4, 5)] and g.checks
    assert g.loop.stop_len.tolist() == [0] * 32 and g.loop.ban_ids.tolist() == [-1] * 32 and g.loop.min_new.tolist() == [0, 0]
    g.loop.generate([[1, 2, 3]], 5, stop=[[40, 41]], stop_token_ids=[42], min_new_tokens=2)
    assert g.loop.stop_len.tolist() == [2] + [0] * 31 and g.loop.stop_ids[0, :3].tolist() == [40, 41, 0] and g.loop.ban_ids[:2].tolist() == [42, -1]
    assert g.loop.min_new[0] == 2


@pytest.mark.parametrize("path", ["host", "decode", "spec"])
def test_an_exception_frees_the_pool_and_leaves_the_loop_idle(monkeypatch, path):
    g = _Paths(path, monkeypatch)
    count = [0]

    def boom(*a, **kw):
        count[0] += 1
        if count[0] >= 3:
            raise RuntimeError("boom")
        return (_stub_ban([]) if path == "host" else _stub_check([]))(*a, **kw)

    monkeypatch.setattr("qqq_amd.model.ops.ban_tokens" if path == "host" else "qqq_amd.serve.ops.stop_check", boom)
    with pytest.raises(RuntimeError, match="boom"):
        g([[1, 2, 3], [0] * 17], 12, stop=[[40, 41]], min_new_tokens=11)
    assert count[0] == 3 and g.cache.free_blocks == 8
    if g.loop is not None:
        assert (g.loop.remaining == 0).all() and (g.loop.pos == -1).all() and (g.loop.slots == -1).all()
        assert g.loop.n_seen.tolist() == (g.loop.n_out + 1).tolist() and g.loop.n_trim.tolist() == [0, 0]


@pytest.mark.parametrize("path", ["host", "decode", "spec"])
def test_eos_and_stop_ids_go_before_a_sequence_that_ends_in_them_on_every_path(monkeypatch, path):
    """a completion that ends in its eos keeps it, also where a stop sequence ends in the same token: as the first token and later"""
    g = _Paths(path, monkeypatch)
    a, b, c = g.up(4, 3)  # the first three tokens behind the prompt [1, 2, 3]: 4, 5, 6 or 4, 0, 1
    for kw, want in ((dict(eos_token_id=c, stop=[[b, c]]), [a, b, c]), (dict(eos_token_id=c, stop=[[c]]), [a, b, c]),
                     (dict(eos_token_id=c, stop=[[a, b, c]]), [a, b, c]), (dict(eos_token_id=a, stop=[[a]]), [a]),
                     (dict(stop_token_ids=[c], stop=[[b, c]]), [a, b, c]), (dict(stop_token_ids=[a], stop=[[a]]), [a]),
                     (dict(eos_token_id=c, stop=[[b, c]], min_new_tokens=2), [a, b, c]), (dict(eos_token_id=c, stop=[[a, b]]), []),
                     (dict(eos_token_id=b, stop_token_ids=[c], stop=[[a, b]]), [a, b])):
        assert g([[1, 2, 3]], 9, **kw) == [want], kw
    assert g.cache.free_blocks == 8


def test_stops_combine_with_families_and_penalties(monkeypatch):
    from test_penalty_cpu import _stub_penalize

    # n = 2 on the host path and DecodeLoop(family=2): greedy siblings are equal; a first-token cut on every sibling, and a later one
    host = _Paths("host", monkeypatch)
    fam = _Paths("decode", monkeypatch, rows=2, family=2)
    prompts = [[1, 2, 3], [7]]
    for kw, want in ((dict(stop=[[4], [10, 11]]), [[[], []], [[8, 9]] * 2]), (dict(stop_token_ids=[8], stop=[[6]]), [[[4, 5]] * 2, [[8]] * 2]),
                     (dict(eos_token_id=10, stop=[[4, 5]], min_new_tokens=4), [[[4, 5, 6, 7, 8, 9]] * 2, [[8, 9, 0, 1, 2, 3]] * 2])):
        assert host(prompts, 6, n=2, **kw) == want, kw
        assert fam(prompts, 6, **kw) == want, kw
        assert host.cache.free_blocks == 8 and fam.cache.free_blocks == 8
    assert (fam.loop.remaining == 0).all() and (fam.loop.shared == 0).all()
    # penalties=True: the ban follows the penalty; presence 2 over the prompt [48, 49, 0, 1] leaves the run 2, 3, 4, ... (test_penalty_cpu)
    pen = _Paths("decode", monkeypatch, penalties=True)
    calls = []
    for mod in ("model", "serve"):
        monkeypatch.setattr(f"qqq_amd.{mod}.ops.penalize_logits", _stub_penalize(calls))
    for kw, want in ((dict(stop=[[10, 11]]), list(range(2, 10))), (dict(stop_token_ids=[6]), [2, 3, 4, 5, 6]),
                     (dict(eos_token_id=4, min_new_tokens=5), [2, 3, 0, 1, 5, 6, 7, 8, 9, 10, 11, 12])):
        got = pen([[48, 49, 0, 1]], 12, presence_penalty=2.0, **kw)
        assert got == [want] and host([[48, 49, 0, 1]], 12, presence_penalty=2.0, **kw) == got, kw
    assert calls and pen.cache.free_blocks == 8
