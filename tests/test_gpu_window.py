"""Sliding-window attention on the GPU (include/qqq_amd_window.h): the windowed paged decode and prefill ops against float64 attention with
the band mask i - W < j <= i, their exact properties (the unwindowed bits at window >= max_len, nothing read behind a window, hipGraph
replay, rows that write nothing), and a Mistral-shaped model: one prefill against chunks and one-token steps, greedy generate with and
without block release, the device loop.  Bounds: relative L2 per (token, head) <= 1e-3 and max error <= 2^-9 max|v| over the keys
attended, those of tests/test_gpu_prefill.py, tests/test_gpu_decode_attn.py and tests/test_gpu_kv8.py for this arithmetic."""
from types import SimpleNamespace

import pytest
import torch

from test_gpu_model import HEADS, HIDDEN, INTER, KVH, LAYERS, VOCAB, _make_lm, _prompts
from test_gpu_paged import SENT, _i32
from test_gpu_prefill import NAN, PAD, STEP, _assert_quant, _cont, _errors, _kv64, _meta, _pools

pytestmark = pytest.mark.gpu

MAX_LEN = 1024


def _ref64(q, k64, v64, seqs, scale, window):
    """float64 attention of the packed tokens q [m, h, d] under the band mask: (out [m, h, d], max |v| over the keys attended [m, h])"""
    h, kvh, dev = q.shape[1], k64.shape[1], q.device
    outs, vmaxs, t = [], [], 0
    for i, (start, c) in enumerate(seqs):
        n = start + c
        k, v = k64[i, :, :n].repeat_interleave(h // kvh, 0), v64[i, :, :n].repeat_interleave(h // kvh, 0)
        s = torch.einsum("thd,hkd->htk", q[t:t + c].double(), k) * scale
        key, pos = torch.arange(n, device=dev)[None], (start + torch.arange(c, device=dev))[:, None]
        keep = (key <= pos) & (key > pos - window)
        outs.append(torch.einsum("htk,hkd->thd", torch.softmax(s.masked_fill(~keep[None], -float("inf")), -1), v))
        vmaxs.append((v.abs().amax(dim=2)[:, None] * keep[None]).amax(dim=2).t())
        t += c
    return torch.cat(outs), torch.cat(vmaxs)


def _op(kind, kv8):
    from qqq_amd import ops

    return getattr(ops, f"{kind}_attention_paged_window" + ("_kv8" if kv8 else ""))


def _decode_positions(h, kvh, window):
    """12 rows: 0 and the window's edge, lo on a 128-key round and on a split's edge, the last position, and filler"""
    from qqq_amd import ops

    chunk = ops.decode_attention_window_plan(12, h, kvh, MAX_LEN, window)[1]
    want = [0, window - 2, window - 1, window, window + 1, 126 + window, 127 + window, 128 + window, chunk - 2 + window, chunk - 1 + window,
            MAX_LEN - 1, 500, 777, 300, 640, 901]
    pos = []
    for p in want:
        if 0 <= p < MAX_LEN and p not in pos:
            pos.append(p)
    return pos[:12], chunk


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("window", [1, 33, 128, 200])
@pytest.mark.parametrize("bs", [16, 256])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,kvh", [(4, 4), (8, 2), (16, 2)])
def test_decode_against_float64(dev, h, kvh, d, bs, window, kv8):
    g = torch.Generator(device=dev).manual_seed(h + d + bs + window)
    pos, chunk = _decode_positions(h, kvh, window)
    assert len(pos) == 12
    lens = [p + 1 for p in pos]
    cont = _cont(dev, g, lens, kvh, d, MAX_LEN, kv8)
    pools, table = _pools(g, cont, lens, bs, kv8)
    q = torch.randn((len(pos), h, d), generator=g, device=dev).half()
    xq, s1, o = _op("decode", kv8)(q, *pools, table, torch.tensor(pos, device=dev), d ** -0.5, window, max_len=MAX_LEN, return_fp16=True)
    assert torch.isfinite(o.float()).all()
    ref, vmax = _ref64(q, *_kv64(cont, kv8), [(p, 1) for p in pos], d ** -0.5, window)
    rel, mx = _errors(o, ref, vmax)
    print(f"decode window={window} chunk={chunk} h={h} kvh={kvh} d={d} bs={bs} kv8={kv8}: rel L2 {rel:.2e}, max|err|/max|v| {mx:.2e}")
    assert rel <= 1e-3 and mx <= 2 ** -9, (rel, mx)
    _assert_quant(xq, s1, o, len(pos), (h, kvh, d, bs, window, kv8))


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("window", [1, 16, 64, 100])
@pytest.mark.parametrize("bs", [16, 128])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,kvh", [(2, 2), (8, 2)])
def test_prefill_against_float64(dev, h, kvh, d, bs, window, kv8):
    """G = 1 with window 16: the 133-token chunk is one query tile whose late rows have whole leading key tiles masked"""
    g = torch.Generator(device=dev).manual_seed(h + d + bs + window)
    lens = [s + c for s, c in STEP]
    cont = _cont(dev, g, lens, kvh, d, MAX_LEN, kv8)
    pools, table = _pools(g, cont, lens, bs, kv8)
    m = sum(c for _, c in STEP)
    q = torch.randn((m + PAD, h, d), generator=g, device=dev).half()
    xq, s1, o = _op("prefill", kv8)(q, *pools, table, *_meta(dev, STEP), d ** -0.5, window, return_fp16=True)
    assert torch.isfinite(o[:m].float()).all() and torch.isfinite(s1[:m]).all()
    ref, vmax = _ref64(q, *_kv64(cont, kv8), STEP, d ** -0.5, window)
    rel, mx = _errors(o[:m], ref, vmax)
    print(f"prefill window={window} h={h} kvh={kvh} d={d} bs={bs} kv8={kv8}: rel L2 {rel:.2e}, max|err|/max|v| {mx:.2e}")
    assert rel <= 1e-3 and mx <= 2 ** -9, (rel, mx)
    _assert_quant(xq, s1, o, m, (h, kvh, d, bs, window, kv8))


H, KV, D, BS, W = 8, 2, 128, 16, 100


def _case(dev, kv8, behind=False):
    """the decode and the prefill call of the exact tests: (decode args, prefill args) over pools that hold the same rows; `behind`: every
    pool row below a row's window is NaN (int8: its scale) and every table entry wholly below it names a block outside the pool"""
    pos = _decode_positions(H, KV, W)[0]
    calls = []
    for seqs in ([(p, 1) for p in pos], STEP):
        g = torch.Generator(device=dev).manual_seed(11)
        lens = [s + c for s, c in seqs]
        cont = [t.clone() for t in _cont(dev, g, lens, KV, D, MAX_LEN, kv8)]
        q = torch.randn((sum(c for _, c in seqs) + PAD, H, D), generator=g, device=dev).half()
        los = [max(0, s - W + 1) for s, _ in seqs]
        if behind:
            for i, lo in enumerate(los):
                for t in cont[2:] if kv8 else cont:
                    t[i, :, :lo] = NAN
        pools, table = _pools(g, tuple(cont), lens, BS, kv8)
        if behind:
            for i, lo in enumerate(los):
                table[i, :lo // BS] = 1 << 30
        calls.append((q, pools, table))
    (qd, pd, td), (qp, pp, tp) = calls
    return ((qd[:len(pos)], *pd, td, torch.tensor(pos, device=dev), D ** -0.5), (qp, *pp, tp, *_meta(dev, STEP), D ** -0.5))


def _same(a, b):
    return all(torch.equal(_i32(x.float()), _i32(y.float())) for x, y in zip(a, b))


@pytest.mark.parametrize("kv8", [False, True])
def test_window_of_max_len_is_the_unwindowed_op_bit_for_bit(dev, kv8):
    from qqq_amd import ops

    dec, pre = _case(dev, kv8)
    m = sum(c for _, c in STEP)
    for window in (MAX_LEN, 1 << 40):
        got = _op("decode", kv8)(*dec, window, max_len=MAX_LEN, return_fp16=True)
        assert _same(got, (ops.decode_attention_paged_kv8 if kv8 else ops.decode_attention_paged)(*dec, max_len=MAX_LEN, return_fp16=True))
        got = _op("prefill", kv8)(*pre, window, max_len=MAX_LEN, return_fp16=True)
        want = (ops.prefill_attention_paged_kv8 if kv8 else ops.prefill_attention_paged)(*pre, max_len=MAX_LEN, return_fp16=True)
        assert _same([t[:m] for t in got], [t[:m] for t in want])


@pytest.mark.parametrize("kv8", [False, True])
def test_nothing_behind_the_window_is_read(dev, kv8):
    m = sum(c for _, c in STEP)
    clean, dirty = _case(dev, kv8), _case(dev, kv8, behind=True)
    for kind, c, d_, rows in (("decode", clean[0], dirty[0], 12), ("prefill", clean[1], dirty[1], m)):
        want = _op(kind, kv8)(*c, W, max_len=MAX_LEN, return_fp16=True)
        got = _op(kind, kv8)(*d_, W, max_len=MAX_LEN, return_fp16=True)
        assert torch.isfinite(got[2][:rows].float()).all() and _same([t[:rows] for t in got], [t[:rows] for t in want]), kind


@pytest.mark.parametrize("kv8", [False, True])
def test_graph_replay_at_other_positions_and_idle_rows(dev, kv8):
    """a captured windowed decode call replayed after pos and the table changed in place equals the eager bits; rows with pos outside
    [0, max_len) and padding tokens leave their sentinel"""
    from qqq_amd import _lib

    dec, pre = _case(dev, kv8)
    *front, table, pos, scale = dec
    L, b = _lib.lib(), pos.numel()
    o = torch.full((b, H * D), SENT, dtype=torch.float16, device=dev)
    xq, s1 = torch.full((b, H * D), 77, dtype=torch.int8, device=dev), torch.full((b, 1), SENT, device=dev)
    ws = torch.empty(L.qqq_decode_attn_window_workspace_bytes(b, H, KV, D, MAX_LEN, W), dtype=torch.uint8, device=dev)
    fn = L.qqq_decode_attn_paged_window_kv8 if kv8 else L.qqq_decode_attn_paged_window
    tab, p = table.clone(), pos.clone()

    def call():
        st = torch.cuda.current_stream().cuda_stream
        assert fn(*(t.data_ptr() for t in front), tab.data_ptr(), tab.shape[1], p.data_ptr(), scale, o.data_ptr(), xq.data_ptr(),
                  s1.data_ptr(), ws.data_ptr(), ws.numel(), b, H, KV, D, front[1].shape[0], BS, MAX_LEN, W, 0, st) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for shift in (0, 1, 5):  # rows move to other rows' positions and tables; two rows go idle
        idx = torch.roll(torch.arange(b, device=dev), shift)
        tab.copy_(table[idx])
        p.copy_(pos[idx])
        p[0], p[1] = -1, MAX_LEN
        o.fill_(SENT), xq.fill_(77), s1.fill_(SENT)
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
        want = _op("decode", kv8)(*front, tab, p, scale, W, max_len=MAX_LEN, return_fp16=True)
        assert _same((xq[2:], s1[2:], o[2:]), [t[2:] for t in want]), shift
        assert (o[:2] == SENT).all() and (xq[:2] == 77).all() and (s1[:2] == SENT).all()
    # prefill through the C entry over sentinel buffers: at max_len 1016 the chunk (1000, 17) does not fit; it and the padding write nothing
    *front, table, cu, sp, scale = pre
    m, n = sum(c for _, c in STEP), front[0].shape[0]
    o = torch.full((n, H * D), SENT, dtype=torch.float16, device=dev)
    xq, s1 = torch.full((n, H * D), 77, dtype=torch.int8, device=dev), torch.full((n, 1), SENT, device=dev)
    fn = L.qqq_prefill_attn_paged_window_kv8 if kv8 else L.qqq_prefill_attn_paged_window
    assert fn(*(t.data_ptr() for t in front), table.data_ptr(), table.shape[1], cu.data_ptr(), sp.data_ptr(), scale, o.data_ptr(),
              xq.data_ptr(), s1.data_ptr(), None, 0, n, len(STEP), H, KV, D, front[1].shape[0], BS, 1016, W, 0,
              torch.cuda.current_stream().cuda_stream) == 0
    want = _op("prefill", kv8)(*pre, W, max_len=MAX_LEN, return_fp16=True)
    idle = torch.zeros(n, dtype=torch.bool, device=dev)
    idle[m:] = True
    idle[sum(c for _, c in STEP[:4]):sum(c for _, c in STEP[:5])] = True
    assert _same((xq[~idle], s1[~idle], o[~idle]), [t[~idle] for t in want])
    assert (o[idle] == SENT).all() and (xq[idle] == 77).all() and (s1[idle] == SENT).all()


# ---- a Mistral-shaped model: every layer windowed

WINDOW = 24


def _mistral(dev, gs=128):
    from qqq_amd import QuantLlamaForCausalLM

    cfg = SimpleNamespace(model_type="mistral", sliding_window=WINDOW, hidden_size=HIDDEN, num_attention_heads=HEADS, num_key_value_heads=KVH,
                          intermediate_size=INTER, rms_norm_eps=1e-6, vocab_size=VOCAB, num_hidden_layers=LAYERS, hidden_act="silu")
    lm = QuantLlamaForCausalLM.from_config(cfg, gs, sliding_window=True).to(dev)
    lm.load_state_dict(_make_lm(dev, gs).state_dict())
    assert [layer.self_attn.sliding_window for layer in lm.model.layers] == [WINDOW] * LAYERS
    return lm.eval()


@pytest.mark.parametrize("dtype", [torch.float16, torch.int8])
def test_one_prefill_equals_chunks_and_one_token_steps(dev, dtype):
    """the prefill kernel on 70 tokens against the same kernel on chunks of 32 and the decode kernel on the last 6: two kernels, one mask"""
    lm = _mistral(dev)
    ids = torch.randint(0, VOCAB, (70,), generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        cache = lm.new_cache(12, 16, dtype)
        cache.add("a")
        whole = lm.model(ids, cache, cache.step(["a"], [70]), all_rows=True)
        cache.add("b")
        parts = [lm.model(ids[s:s + c], cache, cache.step(["b"], [c]), all_rows=True) for s, c in [(0, 32), (32, 32)] + [(64 + i, 1) for i in range(6)]]
    got, want = torch.cat(parts).double(), whole.double()
    rel = ((got - want).norm(dim=1) / want.norm(dim=1)).max().item()
    mx = ((got - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max().item()
    print(f"one prefill against chunks and steps, {dtype}: rel L2 {rel:.2e}, max|err|/max {mx:.2e}")
    assert rel <= 1e-3 and mx <= 2 ** -9, (rel, mx)


def test_generate_releases_blocks_and_the_device_loop_agrees(dev):
    from qqq_amd import PagedKVCache
    from qqq_amd.paged import RELEASED

    held = []

    class Watched(PagedKVCache):
        def release_before(self, seq_id, first_key):
            gone = super().release_before(seq_id, first_key)
            held.append((gone, sum(blk != RELEASED for blk in self._blocks[seq_id])))
            return gone

    lm, prompts, bs = _mistral(dev), _prompts(), 16
    attn = lm.model.layers[0].self_attn
    cache = Watched(LAYERS, 32, attn.num_key_value_heads, attn.head_dim, bs, device=dev)
    released = lm.generate(prompts, 40, cache=cache)
    assert cache.free_blocks == 32 and sum(g for g, _ in held) > 0
    assert max(n for _, n in held) <= -(-WINDOW // bs) + 1  # behind a step: the window's blocks and the current one (one more after step())
    lm.release_blocks = False
    assert lm.generate(prompts, 40) == released
    assert lm.generate(prompts, 40, device_loop=True) == released
