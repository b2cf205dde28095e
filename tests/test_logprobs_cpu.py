"""Per-token top-k log-probabilities without a GPU: what the C ABI's header declares, the two entries' argument
checks (before any launch), the ops' refusals and fake implementations, generate()'s `logprobs` keyword, and the bookkeeping of the
records on the host path and in DecodeLoop with host stubs for the forward pass, the samplers and the two new ops."""
import inspect
import os

import numpy as np
import pytest
import torch

import logprobs_ref
import score_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qqq_amd_logprobs.h")


@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


# ---- the C ABI

def test_the_header_declares_the_two_entries(L):
    from qqq_amd import _abi, _lib, build

    assert _lib.ABI_VERSION == 4 and L.qqq_amd_abi_version() == 4
    protos = _abi.prototypes(HEADER)
    assert set(protos) == {"qqq_topk_logprobs", "qqq_topk_logprobs_step"}
    assert len(protos["qqq_topk_logprobs"][1]) == 12 and len(protos["qqq_topk_logprobs_step"][1]) == 16
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert ret == "int" and fn.restype is __import__("ctypes").c_int and len(fn.argtypes) == len(params), name
        assert all(p.rsplit(" ", 1)[0] in ("const void*", "void*", "int") for p in params), params
    unit = open(build.SRC).read()
    assert '#include "../../include/qqq_amd_logprobs.h"' in unit  # the compiler holds the definitions against the prototypes
    assert unit.index('#include "qqq_score.hip.h"') < unit.index('#include "qqq_logprobs.hip.h"')


def _plain(L, k=5, rows=2, vocab=100, ld=104, logits=None, tokens=None, logprob=None, rank=None, top_ids=None, top=None):
    return L.qqq_topk_logprobs(logits, ld, tokens, logprob, rank, top_ids, top, k, rows, vocab, 0, None)


def _step(L, k=5, rows=2, vocab=100, ld=104, cap=4, out_stride=4, logits=None, top_ids=None, top=None):
    return L.qqq_topk_logprobs_step(logits, ld, None, out_stride, None, None, None, None, top_ids, top, cap, k, rows, vocab, 0, None)


@pytest.mark.parametrize("call,name", [(_plain, b"qqq_topk_logprobs:"), (_step, b"qqq_topk_logprobs_step:")])
def test_bad_arguments_are_refused_before_any_launch(L, call, name):
    buf = np.zeros(4096, np.uint8)
    base = (buf.ctypes.data + 63) & ~63
    for kw in (dict(k=33), dict(k=9, vocab=8, ld=8), dict(vocab=262145, ld=262152), dict(ld=101), dict(k=-1), dict(rows=65536), dict(rows=-1),
               dict(k=0, top_ids=base, top=base + 1024),   # top_ids given with k = 0
               dict(k=0, top_ids=base),
               dict(k=5, logits=base + 2048, top_ids=base),  # ... and one of the pair missing with k > 0
               dict(k=5, logits=base + 2048 + 8, top_ids=base, top=base + 1024),  # misaligned logits
               dict(k=5, logits=base + 2048, top_ids=base + 2, top=base + 1024),
               dict()):                                    # a valid shape with NULL pointers
        assert call(L, **kw) == 17, kw
        assert L.qqq_amd_last_error().startswith(name), (kw, L.qqq_amd_last_error())
    assert call(L, rows=0) == 0  # a no-op, NULL pointers allowed
    if call is _plain:  # nothing asked for; tokens without logprob
        assert _plain(L, k=0, logits=base) == 17 and L.qqq_amd_last_error().startswith(name)
        assert _plain(L, k=0, logits=base, tokens=base + 1024) == 17 and L.qqq_amd_last_error().startswith(name)
    else:
        assert _step(L, logits=base, top_ids=base + 512, top=base + 1024, cap=0) == 17 and L.qqq_amd_last_error().startswith(name)


# ---- the ops layer

def test_ops_are_exported_and_have_no_cpu_path():
    import qqq_amd
    from qqq_amd import ops

    assert qqq_amd.topk_logprobs is ops.topk_logprobs and qqq_amd.topk_logprobs_step is ops.topk_logprobs_step
    assert {"topk_logprobs", "topk_logprobs_step", "TokenLogprobs"} <= set(qqq_amd.__all__)
    logits, tokens = torch.zeros((3, 40), dtype=torch.float16), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.topk_logprobs(logits, tokens, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.topk_logprobs(logits, None, 1)
    i32 = dict(dtype=torch.int32)
    state = dict(out=torch.zeros((3, 4), dtype=torch.int64), n_out=torch.zeros(3, **i32), n_rec=torch.zeros(3, **i32),
                 logprob=torch.zeros((3, 4)), rank=torch.zeros((3, 4), **i32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.topk_logprobs_step(logits, **state)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.topk_logprobs_step(logits, **state, top_ids=torch.zeros((3, 4, 5), **i32), top_logprobs=torch.zeros((3, 4, 5)))
    with pytest.raises(RuntimeError, match="given or None together"):
        ops.topk_logprobs_step(logits, **state, top_ids=torch.zeros((3, 4, 5), **i32))
    with pytest.raises(RuntimeError, match=r"fp16 \[rows, vocab\]"):
        ops.topk_logprobs(torch.zeros(40, dtype=torch.float16), tokens, 5)


def test_fake_implementations_check_dtypes_and_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from qqq_amd import ops

    with FakeTensorMode():
        logits, tokens = torch.zeros((3, 40), dtype=torch.float16), torch.zeros(3, dtype=torch.int64)
        lp, rk, ids, top = ops.topk_logprobs(logits, tokens, 5)
        assert (lp.shape, rk.shape, ids.shape, top.shape) == ((3,), (3,), (3, 5), (3, 5))
        assert (lp.dtype, rk.dtype, ids.dtype, top.dtype) == (torch.float32, torch.int32, torch.int32, torch.float32)
        assert ops.topk_logprobs(logits, tokens, 0)[2:] == (None, None) and ops.topk_logprobs(logits, None, 2)[:2] == (None, None)
        for bad_k in (-1, 33, 41):
            with pytest.raises(ValueError, match="k="):
                ops.topk_logprobs(logits, tokens, bad_k)
        with pytest.raises(ValueError, match="nothing is asked for"):
            ops.topk_logprobs(logits, None, 0)
        with pytest.raises(RuntimeError, match=r"tokens must be int64 \[3\]"):
            ops.topk_logprobs(logits, tokens.int(), 1)
        i32 = dict(dtype=torch.int32)
        state = dict(out=torch.zeros((3, 4), dtype=torch.int64), n_out=torch.zeros(3, **i32), n_rec=torch.zeros(3, **i32),
                     logprob=torch.zeros((3, 4)), rank=torch.zeros((3, 4), **i32))
        assert ops.topk_logprobs_step(logits, **state) is None
        assert ops.topk_logprobs_step(logits, **state, top_ids=torch.zeros((3, 4, 5), **i32), top_logprobs=torch.zeros((3, 4, 5))) is None
        for bad, msg in ((dict(n_rec=torch.zeros(3, dtype=torch.int64)), "n_rec must be int32"), (dict(rank=torch.zeros((3, 5), **i32)), "rank must be"),
                         (dict(out=torch.zeros((2, 4), dtype=torch.int64)), "out must be int64"),
                         (dict(top_ids=torch.zeros((3, 4, 5), **i32), top_logprobs=torch.zeros((3, 4, 4))), "top_logprobs must be")):
            with pytest.raises(RuntimeError, match=msg):
                ops.topk_logprobs_step(logits, **dict(state, **bad))
        with pytest.raises(ValueError, match="k=33"):
            ops.topk_logprobs_step(logits, **state, top_ids=torch.zeros((3, 4, 33), **i32), top_logprobs=torch.zeros((3, 4, 33)))


# ---- generate(): the keyword

def test_logprobs_stands_between_n_and_draft_len_and_is_checked():
    from test_step_cpu import _tiny_lm

    m = _tiny_lm()
    names = list(inspect.signature(m.generate).parameters)
    assert names[names.index("n") + 1] == "logprobs" and names[names.index("logprobs") + 1] == "draft_len"
    assert inspect.signature(m.generate).parameters["logprobs"].default is None
    for bad in (-1, 33):
        with pytest.raises(ValueError, match=f"logprobs={bad}"):
            m.generate([[1, 2]], 3, logprobs=bad)
    with pytest.raises(ValueError, match="logprobs=5 cannot be combined with draft_len=2"):
        m.generate([[1, 2]], 3, logprobs=5, draft_len=2, device_loop=True)
    from qqq_amd import DecodeLoop, SpecDecodeLoop

    assert "logprobs" in inspect.signature(DecodeLoop.__init__).parameters and "logprobs" not in inspect.signature(SpecDecodeLoop.__init__).parameters
    with pytest.raises(ValueError, match="logprobs=33"):
        DecodeLoop(m, m.new_cache(4, 16), rows=2, max_len=32, graph=False, logprobs=33)


def test_generate_passes_logprobs_on_only_when_it_is_set(monkeypatch):
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
    args = ([[1, 2, 3], [4] * 20], 9, 0.5, 7, 0.9, None, 3)
    assert m.generate(*args, device_loop=True) == ["delegated", args, {}]                  # as today
    assert m.generate(*args, device_loop=True, logprobs=None) == ["delegated", args, {}]
    assert m.generate(*args, device_loop=True, n=2) == ["delegated", args, {}]
    assert m.generate(*args, device_loop=True, draft_len=5) == ["delegated", args, {}]
    assert made == [((), {}), ((), {}), ((), dict(family=2)), ((), dict(draft_len=5))]
    del made[:]
    assert m.generate(*args, device_loop=True, logprobs=0) == ["delegated", args, {}]
    assert m.generate(*args, device_loop=True, logprobs=5, n=2, presence_penalty=0.5)[1] == args
    assert made == [((), dict(logprobs=0)), ((), dict(family=2, penalties=True, logprobs=5))]


# ---- the bookkeeping of the records, with host stubs

def _stub_topk(calls):
    """ops.topk_logprobs in torch on the CPU: log_softmax, a rank count and a stable sort"""

    def topk_logprobs(logits, tokens=None, k=0):
        calls.append((logits.shape[0], k))
        x = logits.float()
        ls = x.log_softmax(dim=1)
        order = torch.sort(-x, dim=1, stable=True).indices[:, :k]
        lp = ls.gather(1, tokens[:, None])[:, 0]
        rank = 1 + (x > x.gather(1, tokens[:, None])).sum(dim=1)
        return lp, rank.int(), (order.int() if k else None), (ls.gather(1, order) if k else None)

    return topk_logprobs


def _stub_topk_step(calls):
    plain = _stub_topk([])

    def topk_logprobs_step(logits, out, n_out, n_rec, logprob, rank, top_ids=None, top_logprobs=None):
        wrote = []
        for r in range(logits.shape[0]):
            a, b = int(n_rec[r]), int(n_out[r])
            if 0 <= a < b and a < logprob.shape[1]:
                lp, rk, ids, top = plain(logits[r:r + 1], out[r, a:a + 1], top_ids.shape[2])
                logprob[r, a], rank[r, a] = lp[0], rk[0]
                if top_ids.shape[2]:
                    top_ids[r, a], top_logprobs[r, a] = ids[0], top[0]
                n_rec[r] = a + 1
                wrote.append(r)
        calls.append(wrote)

    return topk_logprobs_step


ONE_HOT = float(1.0 - np.log(np.e + 49.0))  # the stub models' log-probability of their greedy token: one logit at 1, 49 at 0


def _check_records(tokens, records, k):
    """every emitted token has exactly one record, in order: record j's most probable token is token j (the stubs are greedy)"""
    from qqq_amd import TokenLogprobs

    assert len(tokens) == len(records)
    for toks, rec in zip(tokens, records):
        if toks and isinstance(toks[0], list):  # the completions of one prompt
            _check_records(toks, rec, k)
            continue
        assert isinstance(rec, TokenLogprobs) and all(t.device.type == "cpu" for t in rec)
        assert rec.logprob.shape == (len(toks),) and rec.rank.shape == (len(toks),)
        assert rec.top_ids.shape == (len(toks), k) and rec.top_logprobs.shape == (len(toks), k)
        assert rec.logprob.dtype == torch.float32 and rec.rank.dtype == torch.int32 and rec.top_ids.dtype == torch.int32
        assert rec.rank.tolist() == [1] * len(toks)
        assert rec.logprob.tolist() == pytest.approx([ONE_HOT] * len(toks), abs=1e-6)
        if k:
            assert rec.top_ids[:, 0].tolist() == toks
            assert rec.top_logprobs[:, 0].tolist() == pytest.approx([ONE_HOT] * len(toks), abs=1e-6)


def test_host_path_keeps_one_record_per_emitted_token(monkeypatch):
    from test_step_cpu import _LoopStub, _run_up, _tiny_lm

    m = _tiny_lm()
    _LoopStub(m, monkeypatch)
    calls = []
    monkeypatch.setattr("qqq_amd.model.ops.sample_tokens", lambda logits, T, k, p, u: logits.argmax(dim=1))
    monkeypatch.setattr("qqq_amd.model.ops.topk_logprobs", _stub_topk(calls))
    prompts = [[1] * 20, [10] * 3, [30] * 17, [40]]
    plain = m.generate(prompts, 5)
    assert calls == []  # logprobs=None: nothing of it runs
    # two admission waves: a pool of 3 blocks holds the first two prompts, the others wait
    cache = m.new_cache(3, block_size=16)
    toks, recs = m.generate(prompts, 5, cache=cache, logprobs=3)
    assert toks == plain == [_run_up(2, 5), _run_up(11, 5), _run_up(31, 5), _run_up(41, 5)] and cache.free_blocks == 3
    _check_records(toks, recs, 3)
    assert calls[0] == (2, 3) and sum(c[0] for c in calls) == 20 and all(c[1] == 3 for c in calls)  # behind every sampler call
    # an eos in the first token, and one in the middle; k = 0 keeps logprob and rank alone
    del calls[:]
    toks, recs = m.generate([[11], [1], [9]], 4, eos_token_id=12, logprobs=0)
    assert toks == [[12], [2, 3, 4, 5], [10, 11, 12]]
    _check_records(toks, recs, 0)
    # max_new_tokens = 1: the prefill's record alone; 0: none
    toks, recs = m.generate([[1, 2], [7]], 1, logprobs=2)
    assert toks == [[3], [8]]
    _check_records(toks, recs, 2)
    toks, recs = m.generate([[1, 2], [7]], 0, logprobs=2)
    assert toks == [[], []] and [r.top_ids.shape for r in recs] == [(0, 2)] * 2
    assert m.generate([], 3, logprobs=2) == ([], [])
    # n = 3: the nesting of the tokens, the first records from the repeated rows
    del calls[:]
    toks, recs = m.generate([[1, 2, 3], [7]], 4, n=3, logprobs=1, eos_token_id=10)
    assert toks == [[_run_up(4, 4)] * 3, [[8, 9, 10]] * 3] and calls[0] == (6, 1)
    _check_records(toks, recs, 1)


def test_decode_loop_keeps_one_record_per_emitted_token(monkeypatch):
    from qqq_amd import DecodeLoop
    from test_step_cpu import _LoopStub, _run_up, _tiny_lm

    m = _tiny_lm()
    _LoopStub(m, monkeypatch)
    first, steps = [], []
    monkeypatch.setattr("qqq_amd.serve.ops.topk_logprobs", _stub_topk(first))
    monkeypatch.setattr("qqq_amd.serve.ops.topk_logprobs_step", _stub_topk_step(steps))
    cache = m.new_cache(8, 16)
    plain = DecodeLoop(m, cache, rows=2, max_len=48, sync_every=3, u_stride=4, graph=False)
    assert plain.logprobs is None and not any(hasattr(plain, a) for a in ("n_rec", "lp", "lp_rank", "lp_top_ids", "lp_top"))
    prompts = [[1, 2, 3], [10] * 17, [7], [11], [20, 21]]
    want = plain.generate(prompts, 6, eos_token_id=12)
    assert want == [_run_up(4, 6), _run_up(11, 2), _run_up(8, 5), [12], _run_up(22, 6)] and first == [] and steps == []
    loop = DecodeLoop(m, cache, rows=2, max_len=48, sync_every=3, u_stride=4, graph=False, logprobs=4)
    assert loop.logprobs == 4 and loop.n_rec.shape == (2,) and loop.n_rec.dtype == torch.int32
    assert loop.lp.shape == loop.lp_rank.shape == (2, 48) and loop.lp_top_ids.shape == loop.lp_top.shape == (2, 48, 4)
    # more prompts than rows (rows are reused), an eos that ends a row early, an eos in a first token
    toks, recs = loop.generate(prompts, 6, eos_token_id=12)
    assert toks == want and cache.free_blocks == 8
    _check_records(toks, recs, 4)
    assert all(c[1] == 4 for c in first) and sum(c[0] for c in first) == 5 and steps and all(len(w) <= 2 for w in steps)
    assert sum(len(w) for w in steps) == sum(len(t) - 1 for t in toks)  # one record per token the step emitted
    assert loop.n_rec.tolist() == loop.n_out.tolist()
    # again on the same loop, with max_new_tokens = 1 and then 0
    toks, recs = loop.generate([[1], [5], [9]], 1)
    assert toks == [[2], [6], [10]]
    _check_records(toks, recs, 4)
    toks, recs = loop.generate([[1]], 0)
    assert toks == [[]] and recs[0].top_ids.shape == (0, 4)
    # family = 3, k = 0
    fam = DecodeLoop(m, cache, rows=3, max_len=48, sync_every=3, u_stride=4, graph=False, family=3, logprobs=0)
    toks, recs = fam.generate([[1, 2, 3], [7]], 4, eos_token_id=10)
    assert toks == [[_run_up(4, 4)] * 3, [[8, 9, 10]] * 3]
    _check_records(toks, recs, 0)
    # an error in a step leaves no row owing a record
    def boom(*a, **kw):
        raise RuntimeError("boom")

    monkeypatch.setattr("qqq_amd.serve.ops.topk_logprobs_step", boom)
    with pytest.raises(RuntimeError, match="boom"):
        loop.generate([[1, 2]], 5)
    assert loop.n_rec.tolist() == loop.n_out.tolist() and cache.free_blocks == 8


# ---- the reference against itself

def test_reference_agrees_with_the_scoring_reference():
    rng = np.random.default_rng(0)
    row = rng.permutation(np.arange(-300, 300)).astype(np.float16) / 16  # tie-free
    lp, rank, ids, vals = logprobs_ref.topk_logprobs_row(row, 17, 32)
    assert ids[0] == score_ref.token_logprob_row(row, 0)[1] == int(row.argmax())
    assert [logprobs_ref.rank_row(row, int(j)) for j in ids] == list(range(1, 33))
    assert np.all(np.diff(vals) < 0) and lp == score_ref.token_logprob_row(row, 17)[0] and rank == 1 + int((row > row[17]).sum())
    # ties by index, -0 == +0, NaN and -inf last and equal among themselves
    tie = np.array([1.0, np.nan, 2.0, -0.0, 2.0, 0.0, -np.inf, 1.0], np.float16)
    assert logprobs_ref.order(tie).tolist() == [2, 4, 0, 7, 3, 5, 1, 6]
    assert [logprobs_ref.rank_row(tie, t) for t in (2, 4, 0, 3, 5, 1, 6, -1, 8)] == [1, 1, 3, 5, 5, 7, 7, 0, 0]
    lp, rank, ids, vals = logprobs_ref.topk_logprobs_row(tie, 6, 8)
    assert np.isneginf(lp) and np.isneginf(vals[6:]).all() and np.isfinite(vals[:6]).all() and vals[0] == vals[1] and vals[4] == vals[5]
    dead = np.array([np.nan, -np.inf, np.nan], np.float16)
    lp, rank, ids, vals = logprobs_ref.topk_logprobs_row(dead, 1, 2)
    assert np.isnan(lp) and rank == 1 and ids.tolist() == [0, 1] and np.isnan(vals).all()
    out = logprobs_ref.topk_logprobs(np.stack([tie, tie]), None, 3)
    assert out[0] is None and out[1] is None and out[2].tolist() == [[2, 4, 0]] * 2 and out[3].shape == (2, 3)
