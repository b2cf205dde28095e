"""ops.fsm_mask and ops.fsm_advance on the GPU against tests/fsm_ref.py, bit for bit: integer and bit work, so equality is the tolerance.
Every array a case hands to an op lies between two guard regions of a sentinel, and the whole allocation is compared: a write outside
an array, into a pad column or into an allowed column fails the case."""
import numpy as np
import pytest
import torch

import fsm_ref

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = {np.dtype(np.uint16): 0x1234, np.dtype(np.int32): 0x5A5A5A5A, np.dtype(np.int64): 0x5A5A5A5A5A5A5A5A}


class Guarded:
    """a numpy array on the device between two guard regions: .t the tensor the op takes, .host() everything as numpy"""

    def __init__(self, a, dev, lead=GUARD, half=False):
        a = np.ascontiguousarray(a)
        fill = np.full(lead, SENTINEL[a.dtype], a.dtype)
        self.a, self.lead = a, lead
        self.full = torch.from_numpy(np.concatenate([fill, a.reshape(-1), fill[:GUARD]]).view(np.int16 if a.dtype == np.uint16 else a.dtype)).to(dev)
        self.t = self.full[lead:lead + a.size].view(a.shape)
        if half:
            self.t = self.t.view(torch.float16)

    def host(self):
        return self.full.cpu().numpy().view(self.a.dtype)

    def expect(self, a):
        """the whole allocation if the array were `a`"""
        fill = np.full(self.lead, SENTINEL[self.a.dtype], self.a.dtype)
        return np.concatenate([fill, np.ascontiguousarray(a).reshape(-1), fill[:GUARD]])


_AUTOMATA = {}


def _automaton(vocab, rng=None):
    """one automaton per vocab, made once and never changed: a state per kind of edge list; every edge's target is any state"""
    from qqq_amd import TokenFSM

    if vocab in _AUTOMATA:
        return _AUTOMATA[vocab]
    rng = np.random.default_rng(vocab)

    def runs(*spans):
        return sorted({t for a, b in spans for t in range(a, b) if 0 <= t < vocab})

    states = [([], 1), ([], 0), (list(range(vocab)), 0), (runs((0, 1), (vocab - 1, vocab)), 1),
              (runs((5, 12), (60, 70), (127, 129), (250, 262), (2040, 2060), (16380, 16390), (vocab - 9, vocab)), 1),
              (sorted(rng.choice(vocab, size=min(vocab, 37), replace=False).tolist()), 0)]
    if vocab > 100000:  # more edges than one pass of a workgroup takes, over many slices, with a dense stretch of 3000
        states.append((sorted(set(rng.choice(vocab, size=2500, replace=False).tolist()) | set(range(70000, 73000))), 1))
        assert len(states[-1][0]) >= 5000
    tokens = np.array([t for toks, _ in states for t in toks], np.int64)
    offsets = np.cumsum([0] + [len(toks) for toks, _ in states])
    f = TokenFSM(offsets, tokens, rng.integers(0, len(states), size=tokens.shape[0]), [a for _, a in states], 0, vocab)
    _AUTOMATA[vocab] = f
    return f


def _logits(rows, vocab, ld, rng):
    bits = rng.integers(0, 0x10000, size=(rows, ld)).astype(np.uint16)  # any bit pattern: NaN and both infinities among them
    bits[:, vocab:] = 0x4321  # the pad columns
    bits[:, :min(vocab, 4)] = np.array([0x7E00, 0xFC00, 0x7C00, 0xFE01], np.uint16)[:min(vocab, 4)]  # NaN, -inf, +inf, NaN in front
    return bits


def _run_mask(dev, f, bits, vocab, state, eos, remaining, lead=GUARD):
    from qqq_amd import ops

    g = Guarded(bits, dev, lead=lead, half=True)
    gs, ge, gr = Guarded(state, dev), (None if eos is None else Guarded(eos, dev)), (None if remaining is None else Guarded(remaining, dev))
    tables = [Guarded(a, dev) for a in (f.offsets, f.tokens, f.next, f.accept)]
    got = ops.fsm_mask(g.t[:, :vocab], gs.t, tuple(t.t for t in tables), eos=None if ge is None else ge.t,
                       remaining=None if gr is None else gr.t)
    torch.cuda.synchronize()
    assert got.data_ptr() == g.t.data_ptr()
    want = bits.copy()
    fsm_ref.mask(want, state, f.offsets, f.tokens, f.accept, eos=eos, remaining=remaining, vocab=vocab)
    assert np.array_equal(g.host(), g.expect(want))
    for x in [gs, ge, gr] + tables:  # the inputs and their guards are as they were
        assert x is None or np.array_equal(x.host(), x.expect(x.a))
    return want


@pytest.mark.parametrize("rows,vocab,ld,lead", [(1, 1003, 1008, 64), (3, 1003, 1005, 65), (70, 1003, 1008, 64), (70, 1003, 1005, 64), (3, 1, 1, 64),
                                                 (3, 1, 3, 65), (2, 262144, 262144, 64), (2, 262144, 262152, 64), (16, 33000, 33000, 72)])
def test_fsm_mask_equals_the_reference_bit_for_bit(dev, rows, vocab, ld, lead):
    rng = np.random.default_rng(rows * 7 + vocab)
    f = _automaton(vocab, rng)
    S = f.n_states
    bits = _logits(rows, vocab, ld, rng)
    # every state, and -1, -2 and S, over the rows; an eos of -1, an explicit edge, one at or beyond vocab, one that is no edge
    cycle = list(range(S))[::-1] + [-1, -2, S]
    for shift in range(0, len(cycle), max(1, rows)):
        state = np.array([cycle[(shift + r) % len(cycle)] for r in range(rows)], np.int32)
        eos = np.array([(-1, 0, vocab, vocab // 2, vocab - 1, vocab + 7)[(r + shift) % 6] for r in range(rows)], np.int32)
        _run_mask(dev, f, bits, vocab, state, eos, None, lead)
    state = np.array([(2, 4, 0)[r % 3] for r in range(rows)], np.int32)
    _run_mask(dev, f, bits, vocab, state, None, None, lead)  # eos NULL: an accepting state keeps nothing besides its tokens
    remaining = np.array([r % 2 for r in range(rows)], np.int32)  # idle rows are untouched
    _run_mask(dev, f, bits, vocab, state, np.full(rows, vocab - 1, np.int32), remaining, lead)


def _advance_case(rows, rng):
    """rows that meet every rule: 0 -{1}-> 1 (accepting) -{2}-> 2 (terminal), 0 -{3}-> a next out of range, 0 -{4}-> 3 -{5 ... 4004}-> 3"""
    offsets = np.array([0, 3, 4, 4, 4004], np.int32)
    tokens = np.array([1, 3, 4, 2] + list(range(5, 4005)), np.int32)
    nxt = np.array([1, 9, 3, 2] + [3] * 4000, np.int32)
    accept = np.array([0, 1, 0, 1], np.int32)
    kinds = [([1, 2, 0], 2, 0, 0), ([1, 6, 0], 2, 0, 0), ([3, 0, 0], 1, 0, 0), ([1, 7, 0], 2, 0, 0), ([1, 2, 0], 1, 1, 1), ([1, 2, 0], 2, 1, 1),
             ([4, 5, 4004], 3, 0, 0), ([4, 4004, 4005], 3, 1, 3), ([1, 2, 0], 2, 0, -1), ([1, 2, 0], 2, 0, -2), ([1, 2, 0], 2, 0, 4),
             ([6, 0, 0], 1, -3, 1), ([1, 2, 2], 3, 0, 0), ([2 ** 40, 0, 0], 1, 0, 0), ([-1, 0, 0], 1, 0, 3), ([1, 2, 0], 0, 0, 0), ([1, 2, 0], 2, 5, 0)]
    pick = [kinds[r % len(kinds)] for r in range(rows)] if rows >= len(kinds) else [kinds[int(rng.integers(0, len(kinds)))] for _ in range(rows)]
    out = np.array([k[0] for k in pick], np.int64)
    return (offsets, tokens, nxt, accept), out, np.array([k[1] for k in pick], np.int32), np.array([k[2] for k in pick], np.int32), \
        np.array([k[3] for k in pick], np.int32)


def _run_advance(dev, tables, out, n_out, n_fsm, state, eos):
    from qqq_amd import ops

    rows = out.shape[0]
    ids, pos, slots = (np.arange(rows, dtype=np.int64) + base for base in (100, 200, 300))
    remaining = np.full(rows, 3, np.int32)
    names = ("out", "n_out", "n_fsm", "state", "ids", "pos", "slots", "remaining")
    host = dict(zip(names, (out, n_out, n_fsm, state, ids, pos, slots, remaining)))
    g = {k: Guarded(v, dev) for k, v in host.items()}
    ge = None if eos is None else Guarded(eos, dev)
    gt = [Guarded(a, dev) for a in tables]
    ops.fsm_advance(g["out"].t, g["n_out"].t, g["n_fsm"].t, g["state"].t, tuple(t.t for t in gt), g["ids"].t, g["pos"].t, g["slots"].t,
                    g["remaining"].t, eos=None if ge is None else ge.t)
    torch.cuda.synchronize()
    want = {k: v.copy() for k, v in host.items()}
    fsm_ref.advance(want["out"], want["n_out"], want["n_fsm"], want["state"], *tables, want["ids"], want["pos"], want["slots"], want["remaining"],
                    eos=eos)
    for k in names:
        assert np.array_equal(g[k].host(), g[k].expect(want[k])), k
    for x in gt + [ge]:
        assert x is None or np.array_equal(x.host(), x.expect(x.a))
    return want


@pytest.mark.parametrize("rows", [1, 3, 17, 70])
def test_fsm_advance_equals_the_reference(dev, rows):
    rng = np.random.default_rng(rows)
    tables, out, n_out, n_fsm, state = _advance_case(rows, rng)
    want = _run_advance(dev, tables, out, n_out, n_fsm, state, np.full(rows, 6, np.int32))
    if rows == 17:  # the reference itself, rule by rule, in the order of _advance_case's kinds
        assert want["state"].tolist() == [2, 1, -2, -2, 1, 2, 3, -2, -1, -2, 4, 1, -2, -2, -2, 0, 0]
        assert (want["remaining"] == 0).tolist() == [True, False, True, True, False, True, False, True, False, False, False, False, True, True,
                                                     True, False, False]
        assert want["n_fsm"].tolist() == [2, 2, 1, 2, 1, 2, 3, 3, 2, 2, 2, 1, 3, 1, 1, 0, 5]
        assert want["ids"][0] == 0 and want["pos"][0] == want["slots"][0] == -1 and want["ids"][1] == 101
    _run_advance(dev, tables, out, n_out, n_fsm, state, None)  # eos NULL: rule 3 never applies


def test_random_walks_over_a_large_automaton(dev):
    """many rows, a state of 5000 edges and more, several tokens behind per row: the wave's 64-way search against the reference"""
    rng = np.random.default_rng(11)
    f = _automaton(262144, rng)
    rows, width = 70, 4
    state = rng.integers(0, f.n_states, size=rows).astype(np.int32)
    out = np.zeros((rows, width), np.int64)
    for r in range(rows):
        s = int(state[r])
        for i in range(width):
            allowed = f.allowed(s)
            t = int(rng.choice(allowed)) if allowed and rng.random() < 0.8 else int(rng.integers(0, 262144))
            out[r, i] = t
            s = f.step(s, t) if 0 <= s < f.n_states else s
    n_out = rng.integers(0, width + 2, size=rows).astype(np.int32)  # also beyond out_stride
    n_fsm = np.minimum(n_out, rng.integers(0, 3, size=rows)).astype(np.int32)
    _run_advance(dev, (f.offsets, f.tokens, f.next, f.accept), out, n_out, n_fsm, state, rng.integers(-1, 262144, size=rows).astype(np.int32))


def test_both_ops_replay_from_a_captured_graph_with_other_states(dev):
    from qqq_amd import ops

    rng = np.random.default_rng(5)
    rows, vocab = 3, 1003
    f = _automaton(vocab, rng)
    tables = f.tensors(dev)
    first = _logits(rows, vocab, 1008, rng)
    logits = torch.from_numpy(first.view(np.int16)).to(dev).view(torch.float16)
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    state, eos, remaining = torch.tensor([2, 3, 4], **i32), torch.tensor([-1, 7, 500], **i32), torch.ones(rows, **i32)
    out, n_out, n_fsm = torch.zeros((rows, 4), **i64), torch.zeros(rows, **i32), torch.zeros(rows, **i32)
    ids, pos, slots = torch.ones(rows, **i64), torch.ones(rows, **i64), torch.ones(rows, **i64)

    def step():
        ops.fsm_mask(logits[:, :vocab], state, tables, eos=eos, remaining=remaining)
        ops.fsm_advance(out, n_out, n_fsm, state, tables, ids, pos, slots, remaining, eos=eos)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    for trial in range(3):
        st = np.array([(4, 0, 5), (1, 3, -1), (5, 2, 4)][trial], np.int32)
        toks = np.array([[f.allowed(int(s))[0] if f.allowed(int(s)) else 0, 0, 0, 0] for s in st], np.int64)
        bits = _logits(rows, vocab, 1008, rng)
        logits.copy_(torch.from_numpy(bits.view(np.int16)).to(dev).view(torch.float16))
        state.copy_(torch.from_numpy(st))
        out.copy_(torch.from_numpy(toks))
        n_out.fill_(1)
        n_fsm.zero_()
        remaining.fill_(2)
        ids.fill_(9)
        graph.replay()
        torch.cuda.synchronize()
        want = bits.copy()
        fsm_ref.mask(want, st, f.offsets, f.tokens, f.accept, eos=eos.cpu().numpy(), remaining=np.full(rows, 2, np.int32), vocab=vocab)
        assert np.array_equal(logits.cpu().view(torch.int16).numpy().view(np.uint16), want)
        w = dict(state=st.copy(), n_fsm=np.zeros(rows, np.int32), ids=np.full(rows, 9, np.int64), pos=pos.cpu().numpy().copy(),
                 slots=slots.cpu().numpy().copy(), remaining=np.full(rows, 2, np.int32))
        # (pos and slots were read after the replay: only a retiring row's are pinned, below)
        fsm_ref.advance(toks, np.ones(rows, np.int32), w["n_fsm"], w["state"], f.offsets, f.tokens, f.next, f.accept, w["ids"], w["pos"], w["slots"],
                        w["remaining"], eos=eos.cpu().numpy())
        assert state.cpu().numpy().tolist() == w["state"].tolist() and n_fsm.cpu().tolist() == [1] * rows
        assert remaining.cpu().numpy().tolist() == w["remaining"].tolist() and ids.cpu().numpy().tolist() == w["ids"].tolist()
        assert all(p == -1 and s == -1 for p, s, rem in zip(pos.tolist(), slots.tolist(), w["remaining"].tolist()) if rem == 0)


def test_inconsistent_offsets_stay_inside_the_arrays(dev):
    """offsets that descend and point beyond n_edges, tokens that are unsorted and out of range, next out of range: the ops clamp and check,
    so this is an ordinary run -- it returns, and every guard region, pad column and input is as it was.  The mask itself is not pinned."""
    from qqq_amd import ops

    rng = np.random.default_rng(9)
    rows, vocab, ld, E = 5, 1003, 1008, 40
    offsets = np.array([30, 10, 10 ** 9, -5, 2 ** 31 - 1, 0], np.int32)  # 5 states
    tokens = rng.integers(-50, 1100, size=E).astype(np.int32)
    tokens[:4] = [10 ** 6, -3, 2 ** 31 - 1, -2 ** 31]
    nxt = rng.integers(-3, 9, size=E).astype(np.int32)
    accept = np.array([1, 0, 1, 1, 0], np.int32)
    bits = _logits(rows, vocab, ld, rng)
    g = Guarded(bits, dev, half=True)
    state = Guarded(np.arange(rows, dtype=np.int32), dev)
    eos = Guarded(np.array([5, 2000, -7, 1002, 0], np.int32), dev)
    tables = [Guarded(a, dev) for a in (offsets, tokens, nxt, accept)]
    ops.fsm_mask(g.t[:, :vocab], state.t, tuple(t.t for t in tables), eos=eos.t)
    torch.cuda.synchronize()
    got = g.host()
    assert np.array_equal(got[:GUARD], g.expect(bits)[:GUARD]) and np.array_equal(got[-GUARD:], g.expect(bits)[-GUARD:])
    body = got[GUARD:-GUARD].reshape(rows, ld)
    assert (body[:, vocab:] == 0x4321).all() and ((body[:, :vocab] == bits[:, :vocab]) | (body[:, :vocab] == 0xFC00)).all()
    out = Guarded(rng.integers(-5, 1100, size=(rows, 3)).astype(np.int64), dev)
    arrays = {k: Guarded(np.full(rows, v, dt), dev) for k, v, dt in (("n_out", 3, np.int32), ("n_fsm", 0, np.int32), ("ids", 7, np.int64),
                                                                      ("pos", 5, np.int64), ("slots", 9, np.int64), ("remaining", 3, np.int32))}
    ops.fsm_advance(out.t, arrays["n_out"].t, arrays["n_fsm"].t, state.t, tuple(t.t for t in tables), arrays["ids"].t, arrays["pos"].t,
                    arrays["slots"].t, arrays["remaining"].t, eos=eos.t)
    torch.cuda.synchronize()
    for x in [out, eos, arrays["n_out"]] + tables:
        assert np.array_equal(x.host(), x.expect(x.a))
    for x in [state] + [arrays[k] for k in ("n_fsm", "ids", "pos", "slots", "remaining")]:
        h = x.host()
        assert np.array_equal(h[:GUARD], x.expect(x.a)[:GUARD]) and np.array_equal(h[-GUARD:], x.expect(x.a)[-GUARD:])
    assert arrays["n_fsm"].t.tolist() == [3] * rows and all(-2 <= s < 5 for s in state.t.tolist())
