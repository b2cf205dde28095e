"""ops.sample_advance on the GPU: its tokens against ops.sample_tokens bit for bit and its state against tests/step_ref.py after every call,
hipGraph replay with the logits and the state refilled in place, and torch.compile."""
import numpy as np
import pytest
import torch

import step_ref

pytestmark = pytest.mark.gpu

R, VOCAB, LD, BS, WIDTH, OUT, USTRIDE, CALLS = 6, 1003, 1008, 16, 3, 4, 3, 5
STATE = ("tick", "ids", "pos", "slots", "remaining", "out", "n_out")


def _setup(dev):
    """Row 0 greedy, two tokens short of the end of its table; row 1 top-k / top-p, crossing into the table's last block; row 2 idle from the
    start; row 3 draws its eos at the first call; row 4 has one token left; row 5 sits at position 15 and crosses a block boundary."""
    g = torch.Generator(device=dev).manual_seed(23)
    bufs = [torch.zeros((R, LD), dtype=torch.float16, device=dev) for _ in range(CALLS)]
    for b in bufs:
        b[:, :VOCAB] = (3.0 * torch.randn((R, VOCAB), generator=g, device=dev)).half()
        b[:, VOCAB:] = float("inf")  # the padding columns are never read
    par = dict(temperature=torch.tensor([0.0, 0.8, 1.0, 1.0, 1.3, 1.0], device=dev),
               top_k=torch.tensor([0, 50, 0, 0, 0, 7], dtype=torch.int32, device=dev),
               top_p=torch.tensor([1.0, 0.9, 1.0, 1.0, 0.95, 1.0], device=dev),
               u=torch.rand((R, USTRIDE), generator=g, device=dev))
    st = step_ref.new_state(R, WIDTH, OUT, BS)
    st["block_table"][:] = np.random.default_rng(5).permutation(R * WIDTH).reshape(R, WIDTH).astype(np.int32) + 3
    st["pos"][:] = [45, 30, -1, 7, 20, 15]
    st["remaining"][:] = [10, 10, 0, 10, 1, 3]
    st["ids"][:] = [11, 12, 0, 13, 14, 15]
    st["tick"][:] = 0
    st["out"][:] = -7  # what must stay where nothing is emitted
    for r in range(R):
        p = int(st["pos"][r])
        st["slots"][r] = -1 if p < 0 else int(st["block_table"][r, p // BS]) * BS + p % BS
    return bufs, par, st


def _to_dev(st, dev):
    return {k: torch.from_numpy(v).to(dev) for k, v in st.items() if isinstance(v, np.ndarray)}


def _call(ops, logits, par, d):
    ops.sample_advance(logits, par["temperature"], par["top_k"], par["top_p"], par["u"], d["tick"], d["ids"], d["pos"], d["slots"],
                       d["block_table"], d["remaining"], d["eos"], d["out"], d["n_out"], BS)


def _tokens(ops, logits, par, tick):
    """ops.sample_tokens on the same logits with the variate the call indexes"""
    u = par["u"].gather(1, (tick.long() % USTRIDE)[:, None])[:, 0].contiguous()
    return ops.sample_tokens(logits, par["temperature"], par["top_k"], par["top_p"], u)


def _eager_run(dev):
    """the five calls, eagerly: -> (bufs, par, the initial reference state, the device state after each call)"""
    from qqq_amd import ops

    bufs, par, st = _setup(dev)
    st["eos"][3] = int(_tokens(ops, bufs[0][:, :VOCAB], par, torch.zeros(R, dtype=torch.int32, device=dev))[3])
    first = step_ref.copy_state(st)
    d = _to_dev(st, dev)
    after = []
    for i in range(CALLS):
        logits = bufs[i][:, :VOCAB]
        toks = _tokens(ops, logits, par, d["tick"]).tolist()
        before = {k: d[k].clone() for k in STATE}
        _call(ops, logits, par, d)
        torch.cuda.synchronize()
        step_ref.advance(st, toks)
        for k in STATE:
            assert np.array_equal(d[k].cpu().numpy(), st[k]), (i, k, d[k].tolist(), st[k].tolist())
        for r in range(R):  # the token in out IS sample_tokens' token, bit for bit
            if before["remaining"][r] > 0:
                assert d["out"][r, before["n_out"][r]].item() == toks[r], (i, r)
        assert np.array_equal(d["block_table"].cpu().numpy(), st["block_table"]) and np.array_equal(d["eos"].cpu().numpy(), st["eos"])
        after.append({k: d[k].clone() for k in STATE})
    return bufs, par, first, st, after


def test_tokens_equal_sample_tokens_and_state_equals_the_reference_after_every_call(dev):
    _, _, first, st, after = _eager_run(dev)
    # the scenario did what it was built for
    assert st["tick"].tolist() == [CALLS] * R  # 5 calls through u_stride = 3: the variate index wrapped
    assert st["n_out"].tolist() == [3, 4, 0, 1, 1, 3]  # table end, out full, idle, eos, budget 1, budget 3
    assert (st["remaining"] == 0).all() and (st["pos"] == -1).all() and (st["slots"] == -1).all() and (st["ids"] == 0).all()
    assert (st["out"][2] == -7).all() and st["out"][3, 0] == first["eos"][3] and (st["out"][3, 1:] == -7).all()
    a0, a1 = after[0], after[1]
    assert a0["pos"].tolist() == [46, 31, -1, -1, -1, 16] and a1["pos"].tolist()[:2] == [47, 32]
    table = first["block_table"]
    assert a0["slots"][5].item() == int(table[5, 1]) * BS and a1["slots"][1].item() == int(table[1, 2]) * BS
    assert a0["ids"][5].item() == after[0]["out"][5, 0].item()


def test_hipgraph_replays_with_logits_and_state_refilled_in_place(dev):
    from qqq_amd import ops

    bufs, par, first, _, after = _eager_run(dev)
    d = _to_dev(first, dev)
    buf = torch.zeros((R, LD), dtype=torch.float16, device=dev)
    logits = buf[:, :VOCAB]
    buf.copy_(bufs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call(ops, logits, par, d)  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _call(ops, logits, par, d)
    torch.cuda.current_stream().wait_stream(side)
    fresh = _to_dev(first, dev)
    for k in STATE:  # the state again, in place
        d[k].copy_(fresh[k])
    for i in range(CALLS):
        buf.copy_(bufs[i])
        graph.replay()
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(d[k], after[i][k]), (i, k)


def test_sample_advance_traces_under_torch_compile(dev):
    from qqq_amd import ops

    bufs, par, first, _, after = _eager_run(dev)

    def f(logits, T, k, p, u, tick, ids, pos, slots, table, remaining, eos, out, n_out):
        ops.sample_advance(logits * 1, T, k, p, u, tick, ids, pos, slots, table, remaining, eos, out, n_out, BS)
        return pos + 1, n_out * 2

    d = _to_dev(first, dev)
    got = torch.compile(f, fullgraph=True)(bufs[0][:, :VOCAB], par["temperature"], par["top_k"], par["top_p"], par["u"], d["tick"], d["ids"],
                                           d["pos"], d["slots"], d["block_table"], d["remaining"], d["eos"], d["out"], d["n_out"])
    for k in STATE:
        assert torch.equal(d[k], after[0][k]), k
    assert torch.equal(got[0], after[0]["pos"] + 1) and torch.equal(got[1], after[0]["n_out"] * 2)


def test_op_refuses_what_it_cannot_update_in_place(dev):
    from qqq_amd import ops

    bufs, par, first, _, _ = _eager_run(dev)
    d = _to_dev(first, dev)
    wide = torch.zeros((R, 2), dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="pos must be contiguous"):
        _call(ops, bufs[0][:, :VOCAB], par, dict(d, pos=wide[:, 0]))
    with pytest.raises(RuntimeError, match="remaining must be int32"):
        _call(ops, bufs[0][:, :VOCAB], par, dict(d, remaining=d["remaining"].long()))
    with pytest.raises(RuntimeError, match="same GPU|on the GPU"):
        _call(ops, bufs[0][:, :VOCAB], par, dict(d, eos=d["eos"].cpu()))
