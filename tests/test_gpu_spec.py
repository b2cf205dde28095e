"""ops.spec_advance on the GPU: after each of six consecutive calls the whole state against tests/spec_ref.py fed with ops.sample_tokens'
tokens for the same logits rows, parameters and variates, bit for bit; greedy and sampled; draft_len 1, 3 and 15; ngram_max 1, 3 and 4;
and hipGraph replay with the logits and the state refilled in place.

The logits are noise (3 * randn) with a spike of +40 where a draw is steered: its probability is 1 to within e^-30 at any temperature used
here, so the steered draws are the same greedy and sampled, and the scenario below holds in both.  Draws that are not steered are plain
draws from the noise: with the wrong variate they would come out as other tokens."""
import numpy as np
import pytest
import torch

import spec_ref

pytestmark = pytest.mark.gpu

R, VOCAB, LD, BS, WIDTH, HIST, CALLS = 6, 1003, 1008, 16, 4, 64, 6
EOS = 7
STATE = spec_ref.FIELDS
GREEDY, SAMPLED = (0.0, 0, 1.0), (0.8, 50, 0.9)


def _other(d):
    """a token of the histories' alphabet 5 ... 9 that is not d"""
    return 5 + (d - 5 + 1) % 5 if 5 <= d <= 9 else 5


def _initial(k, nmax):
    """Row 0 idle.  Row 1 will accept no draft; row 2 one (its hist has room for four more tokens: it fills up in the second call; the
    kernel takes the position from pos and the length from hist_len, each on its own); row 3 all of them, from position 14 over a block
    boundary; row 4 draws its eos as draw 1 with matching drafts behind it; row 5 has a budget of two."""
    rng = np.random.default_rng(17)
    st = spec_ref.new_state(R, k, WIDTH, HIST, BS)
    table = rng.permutation(R * WIDTH).reshape(R, WIDTH).astype(np.int32) + 3
    st["block_table"][:] = table
    st["hist"][:] = -7  # what must stay where nothing is appended
    spec_ref.seat(st, 1, rng.integers(5, 10, 20).tolist(), table[1], 40, nmax)
    spec_ref.seat(st, 2, rng.integers(5, 10, 60).tolist(), table[2], 40, nmax, pos=30)
    spec_ref.seat(st, 3, [5, 6, 7, 8, 9] * 3, table[3], 40, nmax)
    spec_ref.seat(st, 4, [5, 6, 7, 8, 5], table[4], 40, nmax, eos=EOS)
    spec_ref.seat(st, 5, [9, 8, 9, 8, 9, 8], table[5], 2, nmax)
    assert st["ids"][4, :2].tolist() == [5, 6] and st["ids"][5, :2].tolist() == [8, 9] and st["ids"][3, :2].tolist() == [9, 5]
    return st


def _targets(st, call, k):
    """the steered draws of one call, from the drafts the state holds: {(row, draw): token}"""
    out = {}
    for r in range(R):
        d = st["ids"][r, 1:].tolist()
        if call == 0:
            want = {1: [_other(d[0])], 2: [d[0]] + ([_other(d[1])] if k > 1 else []), 3: d, 4: [d[0], EOS] + d[2:], 5: [9, 8] + d[2:]}.get(r, [])
        else:
            want = d[:min((call + r) % 4, k)]  # that many drafts come true; the draw behind them is a plain draw from the noise
        for j, t in enumerate(want[:k + 1]):
            out[(r, j)] = t
    return out


def _logits(st, call, k, gen, dev):
    buf = torch.zeros((R * (k + 1), LD), dtype=torch.float16, device=dev)
    buf[:, :VOCAB] = (3.0 * torch.randn((R * (k + 1), VOCAB), generator=gen, device=dev)).half()
    buf[:, VOCAB:] = float("inf")  # the padding columns are never read
    for (r, j), t in _targets(st, call, k).items():
        buf[r * (k + 1) + j, t] = 40.0
    return buf


def _to_dev(st, dev):
    return {k: torch.from_numpy(v).to(dev) for k, v in st.items() if isinstance(v, np.ndarray)}


def _call(ops, logits, par, d, nmax):
    ops.spec_advance(logits, par["T"], par["k"], par["p"], par["u"], d["tick"], d["ids"], d["pos"], d["slots"], d["start"], d["block_table"],
                     d["remaining"], d["eos"], d["hist"], d["hist_len"], d["n_out"], d["n_acc"], BS, nmax)


def _tokens(ops, logits, par, tick, g):
    """ops.sample_tokens on the same logits rows with the variates the call indexes -> [R][g]"""
    idx = ((tick.long()[:, None] * g + torch.arange(g, device=tick.device)[None]) % par["u"].shape[1])
    u = par["u"].gather(1, idx).reshape(-1).contiguous()
    return ops.sample_tokens(logits, par["T"], par["k"], par["p"], u).view(-1, g).tolist()


def _eager_run(dev, k, nmax, mode):
    """the six calls, eagerly: -> (the logits of every call, par, the initial state, the reference state, the device state after each)"""
    from qqq_amd import ops

    g = k + 1
    gen = torch.Generator(device=dev).manual_seed(100 * k + nmax)
    par = dict(T=torch.full((R * g,), mode[0], device=dev), k=torch.full((R * g,), mode[1], dtype=torch.int32, device=dev),
               p=torch.full((R * g,), mode[2], device=dev), u=torch.rand((R, 3 * g), generator=gen, device=dev))  # tick wraps u at call 3
    st = _initial(k, nmax)
    first = spec_ref.copy_state(st)
    d = _to_dev(st, dev)
    bufs, after, accepted = [], [], []
    for i in range(CALLS):
        bufs.append(_logits(st, i, k, gen, dev))
        logits = bufs[i][:, :VOCAB]
        toks = _tokens(ops, logits, par, d["tick"], g)
        for (r, j), t in _targets(st, i, k).items():
            assert toks[r][j] == t, (i, r, j)  # the spike steers the draw, greedy or sampled
        before = st["n_acc"].copy()
        _call(ops, logits, par, d, nmax)
        torch.cuda.synchronize()
        spec_ref.advance(st, toks, nmax)
        for f in STATE:
            assert np.array_equal(d[f].cpu().numpy(), st[f]), (i, f, d[f].tolist(), st[f].tolist())
        assert np.array_equal(d["block_table"].cpu().numpy(), st["block_table"]) and np.array_equal(d["eos"].cpu().numpy(), st["eos"])
        after.append({f: d[f].clone() for f in STATE})
        accepted.append((st["n_acc"] - before).tolist())
    return bufs, par, first, st, after, accepted


@pytest.mark.parametrize("mode", [GREEDY, SAMPLED], ids=["greedy", "sampled"])
@pytest.mark.parametrize("k, nmax", [(3, 3), (1, 3), (15, 3), (3, 1), (3, 4)])
def test_state_equals_the_reference_after_every_call(dev, k, nmax, mode):
    _, _, first, st, after, accepted = _eager_run(dev, k, nmax, mode)
    g = k + 1
    a0 = after[0]
    # the scenario of the first call did what it was built for
    assert accepted[0] == [0, 0, min(1, k), k, min(1, k), min(1, k)]
    assert a0["n_out"].tolist() == [0, 1, 1 + min(1, k), g, 2, 2]
    assert a0["remaining"].tolist()[3:] == [40 - g, 0, 0] and a0["start"].tolist()[3:] == [14 + g, -1, -1]
    assert a0["hist"][4, 5:8].tolist() == [6, EOS, -7] and a0["hist_len"][4].item() == 7  # nothing behind the eos, whatever was drafted
    assert a0["hist"][5, 6:9].tolist() == [9, 8, -7]                                        # nor behind the budget's end
    assert a0["pos"][0].tolist() == [-1] * g and (a0["hist"][0] == -7).all() and a0["hist_len"][0].item() == 0  # the idle row
    table = first["block_table"]
    assert a0["slots"][3, 0].item() == int(table[3, (14 + g) // BS]) * BS + (14 + g) % BS and (14 + g) // BS >= 1  # over the boundary
    assert a0["ids"][3, 0].item() == a0["hist"][3, a0["hist_len"][3].item() - 1].item()
    # row 2's hist fills up in the second call: what fits is appended, the row retires
    assert after[1]["hist_len"][2].item() == HIST and after[1]["remaining"][2].item() == 0 and after[0]["remaining"][2].item() > 0
    assert (after[1]["hist"][2] != -7).all()
    assert st["tick"].tolist() == [CALLS] * R and CALLS * g > 3 * g  # six calls through u_stride = 3 g: the variate index wrapped
    if k == 3:  # across the later calls every number of accepted drafts occurred
        assert {a for call in accepted for a in call} == {0, 1, 2, 3}


def test_hipgraph_replays_with_logits_and_state_refilled_in_place(dev):
    from qqq_amd import ops

    k, nmax = 3, 3
    bufs, par, first, _, after, _ = _eager_run(dev, k, nmax, SAMPLED)
    d = _to_dev(first, dev)
    buf = torch.zeros((R * (k + 1), LD), dtype=torch.float16, device=dev)
    logits = buf[:, :VOCAB]
    buf.copy_(bufs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call(ops, logits, par, d, nmax)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _call(ops, logits, par, d, nmax)
    torch.cuda.current_stream().wait_stream(side)
    fresh = _to_dev(first, dev)
    for f in STATE:  # the state again, in place
        d[f].copy_(fresh[f])
    for i in range(CALLS):
        buf.copy_(bufs[i])
        graph.replay()
        torch.cuda.synchronize()
        for f in STATE:
            assert torch.equal(d[f], after[i][f]), (i, f)


def test_op_refuses_what_it_cannot_update_in_place(dev):
    from qqq_amd import ops

    k, nmax = 3, 3
    st = _initial(k, nmax)
    d = _to_dev(st, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    logits = _logits(st, 0, k, gen, dev)[:, :VOCAB]
    par = dict(T=0.0, k=0, p=1.0, u=torch.rand((R, 4), generator=gen, device=dev))
    wide = torch.zeros((R, 8), dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="pos must be contiguous"):
        _call(ops, logits, par, dict(d, pos=wide[:, :4]), nmax)
    with pytest.raises(RuntimeError, match="hist must be int32"):
        _call(ops, logits, par, dict(d, hist=d["hist"].long()), nmax)
    with pytest.raises(RuntimeError, match="same GPU|on the GPU"):
        _call(ops, logits, par, dict(d, eos=d["eos"].cpu()), nmax)
    for f in STATE:
        assert np.array_equal(d[f].cpu().numpy(), st[f]), f  # nothing was touched
