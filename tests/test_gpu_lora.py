"""ops.lora_add on the GPU against tests/lora_ref.py: the derived tolerance, the untouched rows' bits, row invariance, fused against unfused,
a B = 0 adapter, graph replay with the slots rewritten, and the refusals.  The cases (lora_ref.CASES) are the smallest that reach every
path of the kernel: K that is no multiple of a wave's k block (192), Llama-2's down_proj depth (11008), every rank's instance, one to five
token tiles, 16 adapters in one tile, runs across tile boundaries, 1 - 3 parts, and a row stride of y above N."""
import numpy as np
import pytest
import torch

import lora_ref

pytestmark = pytest.mark.gpu

CASES = lora_ref.CASES
IDS = [lora_ref.case_id(c) for c in CASES]


def _dev(d):
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items() if isinstance(v, np.ndarray)}
    t["y"] = t["y"][:, :d["N"]]  # a view: the row stride stays the case's
    return t


def _run(t, cols, y=None, rows=None, slot=None):
    """ops.lora_add on a fresh copy of the case's y (same row stride) -> the result as numpy; `rows`: only those rows, in that order"""
    from qqq_amd import ops

    pick = (lambda a: a) if rows is None else (lambda a: a[rows].contiguous())
    src = t["y"] if y is None else y
    buf = torch.empty((len(rows) if rows is not None else src.shape[0], src.stride(0)), dtype=torch.float16, device="cuda")
    out = buf[:, :src.shape[1]]
    out.copy_(src if rows is None else src[rows])
    ops.lora_add(out, pick(t["xq"]), pick(t["s1"]), t["A"], t["B"], t["scale"], pick(t["slot"]) if slot is None else slot, cols)
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def refs():
    """per case: its operands, the f64 reference with its bound (computed once, never modified) and the op's result on the whole batch"""
    from qqq_amd import _lib

    _lib.lib()
    out = {}
    for c, cid in zip(CASES, IDS):
        d = lora_ref.inputs(c)
        val, bound, touched = lora_ref.reference(d["y"][:, :d["N"]], d["xq"], d["s1"], d["A"], d["B"], d["scale"], d["slot"], d["part_cols"])
        t = _dev(d)
        out[cid] = dict(d=d, t=t, val=val, bound=bound, touched=touched, got=_run(t, d["part_cols"]))
    return out


@pytest.mark.parametrize("cid", IDS)
def test_within_the_derived_tolerance_and_untouched_rows_keep_their_bits(refs, cid):
    r = refs[cid]
    ok = lora_ref.check(r["got"], r["val"], r["bound"])
    worst = np.abs(r["got"].astype(np.float64) - r["val"]) / lora_ref.fp16_ulp(r["got"].astype(np.float64))
    print(f"{cid}: {int((~ok).sum())} of {ok.size} outside; largest distance {worst.max():.3f} fp16 ulp")
    assert ok.all(), np.argwhere(~ok)[:8]
    y0 = r["d"]["y"][:, :r["d"]["N"]]
    assert np.array_equal(r["got"][~r["touched"]].view(np.uint16), y0[~r["touched"]].view(np.uint16))
    if r["touched"].any():  # the adapters do something: a kernel that leaves y alone fails here
        assert not np.array_equal(r["got"][r["touched"]], y0[r["touched"]])


def test_rows_without_a_slot_keep_negative_zero_and_nan_payloads():
    c = (17, 128, 128, 16, (0, 128), "interleaved", 128)
    d = lora_ref.inputs(c)
    bits = d["y"].view(np.uint16)
    bits[0, :4] = [0x8000, 0x7E01, 0xFD55, 0x7C00]  # -0, two NaN payloads, +inf, on a row of slot -1
    assert d["slot"][0] == -1
    t = _dev(d)
    for slot in (None, torch.tensor([-1, 17, -5, 2 ** 30, -2 ** 31] + [99] * 12, dtype=torch.int32, device="cuda")):
        got = _run(t, c[4], slot=slot)
        keep = d["slot"] < 0 if slot is None else np.ones(17, dtype=bool)  # a slot outside [-1, S) counts as -1
        assert np.array_equal(got[keep].view(np.uint16), d["y"][keep].view(np.uint16))


@pytest.mark.parametrize("cid", IDS)
def test_a_row_alone_and_the_batch_reversed_give_the_same_bits(refs, cid):
    r = refs[cid]
    T = r["got"].shape[0]
    cols = r["d"]["part_cols"]
    rev = _run(r["t"], cols, rows=torch.arange(T - 1, -1, -1, device="cuda"))
    assert np.array_equal(rev[::-1].view(np.uint16), r["got"].view(np.uint16))
    for row in range(T):
        alone = _run(r["t"], cols, rows=torch.tensor([row], device="cuda"))
        assert np.array_equal(alone[0].view(np.uint16), r["got"][row].view(np.uint16)), row


@pytest.mark.parametrize("cid", [i for c, i in zip(CASES, IDS) if len(c[4]) > 2])
def test_fused_and_unfused_give_the_same_bits(refs, cid):
    from qqq_amd import ops

    r = refs[cid]
    t, cols = r["t"], r["d"]["part_cols"]
    R = t["B"].shape[2]
    y = torch.empty((t["y"].shape[0], t["y"].stride(0)), dtype=torch.float16, device="cuda")[:, :t["y"].shape[1]]
    y.copy_(t["y"])
    for p in range(len(cols) - 1):
        ops.lora_add(y[:, cols[p]:cols[p + 1]], t["xq"], t["s1"], t["A"][:, p * R:(p + 1) * R], t["B"][:, cols[p]:cols[p + 1]], t["scale"],
                     t["slot"])
    assert np.array_equal(y.cpu().numpy().view(np.uint16), r["got"].view(np.uint16))


def test_an_adapter_with_b_zero_leaves_y_equal_as_numbers(refs):
    r = refs[IDS[4]]
    t = dict(r["t"], B=torch.zeros_like(r["t"]["B"]))
    got = _run(t, r["d"]["part_cols"])
    assert np.array_equal(got, r["d"]["y"][:, :r["d"]["N"]])


def test_graph_replay_with_the_slots_rewritten_equals_the_eager_calls(refs):
    from qqq_amd import ops

    r = refs[IDS[8]]
    t, cols = r["t"], r["d"]["part_cols"]
    T = t["y"].shape[0]
    other = torch.from_numpy(lora_ref.slots_of("runs", T)).cuda()
    eager = [r["got"], _run(t, cols, slot=other)]
    y, slot = t["y"].clone(), t["slot"].clone()
    ops.lora_add(y, t["xq"], t["s1"], t["A"], t["B"], t["scale"], slot, cols)  # warm-up outside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.lora_add(y, t["xq"], t["s1"], t["A"], t["B"], t["scale"], slot, cols)
    for want, s in zip(eager, (t["slot"], other)):
        y.copy_(t["y"])
        slot.copy_(s)
        g.replay()
        assert np.array_equal(y.cpu().numpy().view(np.uint16), want.view(np.uint16))


def test_refusals():
    from qqq_amd import ops

    d = lora_ref.inputs((4, 128, 128, 16, (0, 128), "same", 128))
    t = _dev(d)
    call = lambda cols=(0, 128), **kw: ops.lora_add(*[kw.get(k, t[k]) for k in ("y", "xq", "s1", "A", "B", "scale", "slot")], cols)  # noqa: E731
    before = t["y"].clone()
    for name, dtype in (("y", torch.float32), ("xq", torch.int32), ("s1", torch.float16), ("A", torch.float32), ("B", torch.float32),
                        ("scale", torch.float16), ("slot", torch.int64)):
        with pytest.raises(RuntimeError, match=f"lora_add: {name} must be "):
            call(**{name: t[name].to(dtype)})
    with pytest.raises(RuntimeError, match="qqq_lora_add: R=24 is not one of 8, 16, 32, 64"):
        call(A=torch.zeros((17, 24, 128), dtype=torch.float16, device="cuda"), B=torch.zeros((17, 128, 24), dtype=torch.float16, device="cuda"))
    for cols in ((0, 64), (64, 128), (0, 96, 128), (0, 128, 128), (0, 64, 64, 128)):
        with pytest.raises(RuntimeError, match="(qqq_lora_add: part_cols must ascend strictly from 0 to N=128 in multiples of 64|lora_add: with y)"):
            call(cols)
    with pytest.raises(RuntimeError, match="qqq_lora_add: bad argument .*aligned"):
        call(xq=torch.zeros(4 * 128 + 8, dtype=torch.int8, device="cuda")[8:].reshape(4, 128))
    with pytest.raises(RuntimeError, match="lora_add: y must have unit column stride"):
        call(y=torch.zeros((128, 4), dtype=torch.float16, device="cuda").t())
    with pytest.raises(RuntimeError, match="qqq_lora_add: bad shape .*ldy=129"):
        call(y=torch.zeros((4, 129), dtype=torch.float16, device="cuda")[:, :128])
    with pytest.raises(RuntimeError, match="lora_add: A and B must have contiguous rows"):
        call(A=torch.zeros((17, 128, 16), dtype=torch.float16, device="cuda").transpose(1, 2))
    with pytest.raises(RuntimeError, match="lora_add: s1 must be f32"):
        call(slot=t["slot"][:3])
    with pytest.raises(RuntimeError, match="every tensor must be on the GPU"):
        call(slot=t["slot"].cpu())
    torch.cuda.synchronize()
    assert torch.equal(t["y"], before)  # nothing was launched
