"""The ops layer's messages, to the letter: every check of the sampler family that needs no GPU (_sample_advance_check,
_spec_advance_check and _token_logprobs_check on CPU and meta tensors, and what the public wrappers refuse before them) and the refusal
of CPU tensors by every op that has one.  MESSAGES was recorded from the commit before the checks were folded into shared helpers.

    python tests/test_ops_messages_cpu.py --print    prints the table's source as the working tree's ops.py gives it"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

f16, f32, f64, i32, i64 = torch.float16, torch.float32, torch.float64, torch.int32, torch.int64


def z(*shape, dtype=f32, device="cpu"):
    return torch.zeros(shape, dtype=dtype, device=device)


# ---- the arguments of a good call, as a dict: a case replaces some of them

def _advance_args(rows=3, vocab=40, device="cpu"):
    kw = dict(device=device)
    return dict(logits=z(rows, vocab, dtype=f16, **kw), temperature=z(rows, **kw), top_k=z(rows, dtype=i32, **kw), top_p=z(rows, **kw),
                u=z(rows, 2, **kw), tick=z(rows, dtype=i32, **kw), ids=z(rows, dtype=i64, **kw), pos=z(rows, dtype=i64, **kw),
                slots=z(rows, dtype=i64, **kw), block_table=z(rows, 2, dtype=i32, **kw), remaining=z(rows, dtype=i32, **kw),
                eos=z(rows, dtype=i32, **kw), out=z(rows, 5, dtype=i64, **kw), n_out=z(rows, dtype=i32, **kw), block_size=16)


def _spec_args(rows=3, group=3, vocab=40, device="cpu"):
    kw, m = dict(device=device), rows * group
    return dict(logits=z(m, vocab, dtype=f16, **kw), temperature=z(m, **kw), top_k=z(m, dtype=i32, **kw), top_p=z(m, **kw),
                u=z(rows, 2 * group, **kw), tick=z(rows, dtype=i32, **kw), ids=z(rows, group, dtype=i64, **kw), pos=z(rows, group, dtype=i64, **kw),
                slots=z(rows, group, dtype=i64, **kw), start=z(rows, dtype=i64, **kw), block_table=z(rows, 2, dtype=i32, **kw),
                remaining=z(rows, dtype=i32, **kw), eos=z(rows, dtype=i32, **kw), hist=z(rows, 9, dtype=i32, **kw),
                hist_len=z(rows, dtype=i32, **kw), n_out=z(rows, dtype=i32, **kw), n_acc=z(rows, dtype=i32, **kw), block_size=16,
                ngram_max=3)


def _logprob_args(rows=3, vocab=40, device="cpu"):
    return dict(logits=z(rows, vocab, dtype=f16, device=device), targets=z(rows, dtype=i64, device=device))


def _bad_state(args, names):
    # every row-state array with another dtype, another rank and another row count
    for name in names:
        t = args[name]
        yield f"{name}-dtype", {name: t.to(f64)}
        yield f"{name}-rank", {name: t[:, None] if t.dim() == 1 else t[0]}
        yield f"{name}-rows", {name: torch.cat((t, t[:1]))}


def _sampler_cases(prefix, args, m):
    # the checks the three sampler-family ops have in common; m: the logits rows
    yield f"{prefix}/logits-dtype", dict(logits=args["logits"].float())
    yield f"{prefix}/logits-rank", dict(logits=args["logits"][0])
    for name in ("temperature", "top_k", "top_p", "u"):
        yield f"{prefix}/{name}-dtype", {name: args[name].to(f64)}
    for name, dtype in (("temperature", f32), ("top_k", i32), ("top_p", f32)):
        yield f"{prefix}/{name}-count", {name: z(m + 1, dtype=dtype)}
    yield f"{prefix}/u-rank", dict(u=args["u"][0])
    yield f"{prefix}/u-rows", dict(u=torch.cat((args["u"], args["u"][:1])))
    yield f"{prefix}/u-stride", dict(u=args["u"][:, :0])
    yield f"{prefix}/block_table-dtype", dict(block_table=args["block_table"].long())
    yield f"{prefix}/block_table-rank", dict(block_table=args["block_table"][0])
    yield f"{prefix}/block_table-rows", dict(block_table=args["block_table"][:2])
    yield f"{prefix}/block_table-width", dict(block_table=args["block_table"][:, :0])
    for b in (24, 8, 512):
        yield f"{prefix}/block_size-{b}", dict(block_size=b)
    yield f"{prefix}/vocab-0", dict(logits=args["logits"][:, :0])


def _cases():
    """(id, callable, its keyword arguments)"""
    from qqq_amd import ops

    def check(fn, good, bad):
        return fn, dict(good, **bad)

    # _sample_advance_check
    a = _advance_args()
    for cid, bad in _sampler_cases("advance", a, 3):
        yield (cid,) + check(ops._sample_advance_check, a, bad)
    for cid, bad in _bad_state(a, [n for n, _ in ops._ADVANCE_STATE]):
        yield (f"advance/{cid}",) + check(ops._sample_advance_check, a, bad)
    for cid, bad in (("out-dtype", dict(out=a["out"].int())), ("out-rank", dict(out=a["out"][0])), ("out-rows", dict(out=a["out"][:2])),
                     ("out-width", dict(out=a["out"][:, :0]))):
        yield (f"advance/{cid}",) + check(ops._sample_advance_check, a, bad)
    yield ("advance/vocab-262145",) + check(ops._sample_advance_check, _advance_args(1, 262145, "meta"), {})
    yield ("advance/rows-65536",) + check(ops._sample_advance_check, _advance_args(65536, 8, "meta"), {})
    # _spec_advance_check
    s = _spec_args()
    for cid, bad in _sampler_cases("spec", s, 9):
        yield (cid,) + check(ops._spec_advance_check, s, bad)
    for cid, bad in _bad_state(s, [n for n, _ in ops._SPEC_ROW_STATE]):
        yield (f"spec/{cid}",) + check(ops._spec_advance_check, s, bad)
    for cid, bad in (("ids-dtype", dict(ids=s["ids"].int())), ("ids-rank", dict(ids=s["ids"][0])), ("ids-group-1", dict(ids=z(3, 1, dtype=i64))),
                     ("ids-group-17", dict(ids=z(3, 17, dtype=i64))), ("logits-rows", dict(logits=z(8, 40, dtype=f16))),
                     ("u-short", dict(u=s["u"][:, :2])), ("pos-dtype", dict(pos=s["pos"].int())), ("pos-shape", dict(pos=s["pos"][:, :2])),
                     ("slots-dtype", dict(slots=s["slots"].int())), ("slots-shape", dict(slots=s["slots"][:2])),
                     ("hist-dtype", dict(hist=s["hist"].long())), ("hist-rank", dict(hist=s["hist"][0])), ("hist-rows", dict(hist=s["hist"][:2])),
                     ("hist-width", dict(hist=s["hist"][:, :0])), ("ngram_max-0", dict(ngram_max=0)), ("ngram_max-5", dict(ngram_max=5))):
        yield (f"spec/{cid}",) + check(ops._spec_advance_check, s, bad)
    yield ("spec/vocab-262145",) + check(ops._spec_advance_check, _spec_args(1, 2, 262145, "meta"), {})
    yield ("spec/rows-65536",) + check(ops._spec_advance_check, _spec_args(4096, 16, 8, "meta"), {})
    # _token_logprobs_check
    t = _logprob_args()
    for cid, bad in (("logits-dtype", dict(logits=t["logits"].float())), ("logits-rank", dict(logits=t["logits"][0])),
                     ("targets-dtype", dict(targets=t["targets"].int())), ("targets-rank", dict(targets=t["targets"][:, None])),
                     ("targets-rows", dict(targets=t["targets"][:2])), ("vocab-0", dict(logits=t["logits"][:, :0]))):
        yield (f"logprobs/{cid}",) + check(ops._token_logprobs_check, t, bad)
    yield ("logprobs/vocab-262145",) + check(ops._token_logprobs_check, _logprob_args(1, 262145, "meta"), {})
    yield ("logprobs/rows-1048577",) + check(ops._token_logprobs_check, _logprob_args(1048577, 8, "meta"), {})
    # what the public wrappers refuse before any of that
    tok = dict(logits=a["logits"], temperature=1.0, top_k=0, top_p=1.0, u=z(3))
    for prefix, fn, good in (("sample_tokens", ops.sample_tokens, tok), ("sample_advance", ops.sample_advance, a), ("spec_advance", ops.spec_advance, s)):
        yield (f"{prefix}/no-tensor",) + check(fn, good, dict(logits=[[0.0]]))
        yield (f"{prefix}/u-no-tensor",) + check(fn, good, dict(u=None))
        yield (f"{prefix}/logits-rank",) + check(fn, good, dict(logits=good["logits"][0]))
        yield (f"{prefix}/temperature-count",) + check(fn, good, dict(temperature=z(2)))
        yield (f"{prefix}/top_k-count",) + check(fn, good, dict(top_k=z(2, dtype=i32)))
        yield (f"{prefix}/top_p-device",) + check(fn, good, dict(top_p=z(1, device="meta")))
    yield ("spec_advance/ids-no-tensor",) + check(ops.spec_advance, s, dict(ids=None))
    yield ("token_logprobs/no-tensor",) + check(ops.token_logprobs, t, dict(targets=[0, 0, 0]))
    yield ("token_logprobs/logits-rank",) + check(ops.token_logprobs, t, dict(logits=t["logits"][0]))
    # CPU tensors: every op that asks for "every tensor on the GPU", and token_logprobs' own wording
    h = z(2, 128, dtype=f16)
    cos, pos, slots = z(8, 64, dtype=f16), z(2, dtype=i64), z(2, dtype=i64)
    cache, scale = z(2, 1, 16, 64, dtype=f16), z(2, 1, 16)
    cache8, q_out, table = cache.to(torch.int8), z(2, 2, 1, 64, dtype=f16), z(2, 1, dtype=i32)
    cu = z(3, dtype=i32)
    yield "cpu/rope_qkv", ops.rope_qkv, dict(q=h, k=h, v=h, cos=cos, sin=cos, pos=pos, k_cache=cache, v_cache=cache)
    yield "cpu/decode_attention", ops.decode_attention, dict(q_out=q_out, k_cache=cache, v_cache=cache, pos=pos, scale=1.0)
    yield "cpu/rope_qkv_kv8", ops.rope_qkv_kv8, dict(q=h, k=h, v=h, cos=cos, sin=cos, pos=pos, k_cache=cache8, v_cache=cache8, k_scale=scale,
                                                    v_scale=scale)
    yield "cpu/decode_attention_kv8", ops.decode_attention_kv8, dict(q_out=q_out, k_cache=cache8, v_cache=cache8, k_scale=scale,
                                                                    v_scale=scale, pos=pos, scale=1.0)
    yield "cpu/rope_qkv_paged", ops.rope_qkv_paged, dict(q=h, k=h, v=h, cos=cos, sin=cos, pos=pos, slots=slots, k_pool=cache, v_pool=cache)
    yield "cpu/rope_qkv_paged_kv8", ops.rope_qkv_paged_kv8, dict(q=h, k=h, v=h, cos=cos, sin=cos, pos=pos, slots=slots, k_pool=cache8,
                                                                v_pool=cache8, k_scale=scale, v_scale=scale)
    yield "cpu/decode_attention_paged", ops.decode_attention_paged, dict(q_out=q_out, k_pool=cache, v_pool=cache, block_table=table, pos=pos,
                                                                        scale=1.0)
    yield "cpu/decode_attention_paged_kv8", ops.decode_attention_paged_kv8, dict(q_out=q_out, k_pool=cache8, v_pool=cache8, k_scale=scale,
                                                                                v_scale=scale, block_table=table, pos=pos, scale=1.0)
    yield "cpu/prefill_attention_paged", ops.prefill_attention_paged, dict(q_out=q_out[:, :, 0], k_pool=cache, v_pool=cache, block_table=table,
                                                                          cu_tokens=cu, start_pos=pos, scale=1.0)
    yield "cpu/prefill_attention_paged_kv8", ops.prefill_attention_paged_kv8, dict(q_out=q_out[:, :, 0], k_pool=cache8, v_pool=cache8,
                                                                                  k_scale=scale, v_scale=scale, block_table=table,
                                                                                  cu_tokens=cu, start_pos=pos, scale=1.0)
    yield "cpu/sample_tokens", ops.sample_tokens, tok
    yield "cpu/sample_advance", ops.sample_advance, a
    yield "cpu/spec_advance", ops.spec_advance, s
    yield "cpu/token_logprobs", ops._token_logprobs_impl, dict(t, return_argmax=True)


def _message(fn, kwargs):
    with pytest.raises(RuntimeError) as e:
        fn(**kwargs)
    return str(e.value)


MESSAGES = {
    'advance/logits-dtype': 'sample_advance: logits must be fp16 [rows, vocab]',
    'advance/logits-rank': 'sample_advance: logits must be fp16 [rows, vocab]',
    'advance/temperature-dtype': 'sample_advance: temperature, top_p and u must be f32, top_k int32',
    'advance/top_k-dtype': 'sample_advance: temperature, top_p and u must be f32, top_k int32',
    'advance/top_p-dtype': 'sample_advance: temperature, top_p and u must be f32, top_k int32',
    'advance/u-dtype': 'sample_advance: temperature, top_p and u must be f32, top_k int32',
    'advance/temperature-count': 'sample_advance: temperature, top_k and top_p must hold one entry per row (3)',
    'advance/top_k-count': 'sample_advance: temperature, top_k and top_p must hold one entry per row (3)',
    'advance/top_p-count': 'sample_advance: temperature, top_k and top_p must hold one entry per row (3)',
    'advance/u-rank': 'sample_advance: u must be f32 [3, u_stride] with u_stride >= 1, not (2,)',
    'advance/u-rows': 'sample_advance: u must be f32 [3, u_stride] with u_stride >= 1, not (4, 2)',
    'advance/u-stride': 'sample_advance: u must be f32 [3, u_stride] with u_stride >= 1, not (3, 0)',
    'advance/block_table-dtype': 'sample_advance: block_table must be int32 [3, blocks per row >= 1], not (3, 2)',
    'advance/block_table-rank': 'sample_advance: block_table must be int32 [3, blocks per row >= 1], not (2,)',
    'advance/block_table-rows': 'sample_advance: block_table must be int32 [3, blocks per row >= 1], not (2, 2)',
    'advance/block_table-width': 'sample_advance: block_table must be int32 [3, blocks per row >= 1], not (3, 0)',
    'advance/block_size-24': 'sample_advance: block_size must be a power of two in [16, 256], not 24',
    'advance/block_size-8': 'sample_advance: block_size must be a power of two in [16, 256], not 8',
    'advance/block_size-512': 'sample_advance: block_size must be a power of two in [16, 256], not 512',
    'advance/vocab-0': 'sample_advance: logits (3, 0) outside 1 <= vocab <= 262144, rows <= 65535',
    'advance/tick-dtype': 'sample_advance: tick must be int32 [3], not float64 (3,)',
    'advance/tick-rank': 'sample_advance: tick must be int32 [3], not int32 (3, 1)',
    'advance/tick-rows': 'sample_advance: tick must be int32 [3], not int32 (4,)',
    'advance/ids-dtype': 'sample_advance: ids must be int64 [3], not float64 (3,)',
    'advance/ids-rank': 'sample_advance: ids must be int64 [3], not int64 (3, 1)',
    'advance/ids-rows': 'sample_advance: ids must be int64 [3], not int64 (4,)',
    'advance/pos-dtype': 'sample_advance: pos must be int64 [3], not float64 (3,)',
    'advance/pos-rank': 'sample_advance: pos must be int64 [3], not int64 (3, 1)',
    'advance/pos-rows': 'sample_advance: pos must be int64 [3], not int64 (4,)',
    'advance/slots-dtype': 'sample_advance: slots must be int64 [3], not float64 (3,)',
    'advance/slots-rank': 'sample_advance: slots must be int64 [3], not int64 (3, 1)',
    'advance/slots-rows': 'sample_advance: slots must be int64 [3], not int64 (4,)',
    'advance/remaining-dtype': 'sample_advance: remaining must be int32 [3], not float64 (3,)',
    'advance/remaining-rank': 'sample_advance: remaining must be int32 [3], not int32 (3, 1)',
    'advance/remaining-rows': 'sample_advance: remaining must be int32 [3], not int32 (4,)',
    'advance/eos-dtype': 'sample_advance: eos must be int32 [3], not float64 (3,)',
    'advance/eos-rank': 'sample_advance: eos must be int32 [3], not int32 (3, 1)',
    'advance/eos-rows': 'sample_advance: eos must be int32 [3], not int32 (4,)',
    'advance/n_out-dtype': 'sample_advance: n_out must be int32 [3], not float64 (3,)',
    'advance/n_out-rank': 'sample_advance: n_out must be int32 [3], not int32 (3, 1)',
    'advance/n_out-rows': 'sample_advance: n_out must be int32 [3], not int32 (4,)',
    'advance/out-dtype': 'sample_advance: out must be int64 [3, out_stride >= 1], not (3, 5)',
    'advance/out-rank': 'sample_advance: out must be int64 [3, out_stride >= 1], not (5,)',
    'advance/out-rows': 'sample_advance: out must be int64 [3, out_stride >= 1], not (2, 5)',
    'advance/out-width': 'sample_advance: out must be int64 [3, out_stride >= 1], not (3, 0)',
    'advance/vocab-262145': 'sample_advance: logits (1, 262145) outside 1 <= vocab <= 262144, rows <= 65535',
    'advance/rows-65536': 'sample_advance: logits (65536, 8) outside 1 <= vocab <= 262144, rows <= 65535',
    'spec/logits-dtype': 'spec_advance: logits must be fp16 [rows * (draft_len + 1), vocab]',
    'spec/logits-rank': 'spec_advance: logits must be fp16 [rows * (draft_len + 1), vocab]',
    'spec/temperature-dtype': 'spec_advance: temperature, top_p and u must be f32, top_k int32',
    'spec/top_k-dtype': 'spec_advance: temperature, top_p and u must be f32, top_k int32',
    'spec/top_p-dtype': 'spec_advance: temperature, top_p and u must be f32, top_k int32',
    'spec/u-dtype': 'spec_advance: temperature, top_p and u must be f32, top_k int32',
    'spec/temperature-count': 'spec_advance: temperature, top_k and top_p must hold one entry per logits row (9)',
    'spec/top_k-count': 'spec_advance: temperature, top_k and top_p must hold one entry per logits row (9)',
    'spec/top_p-count': 'spec_advance: temperature, top_k and top_p must hold one entry per logits row (9)',
    'spec/u-rank': 'spec_advance: u must be f32 [3, u_stride] with u_stride >= draft_len + 1 = 3, not (6,)',
    'spec/u-rows': 'spec_advance: u must be f32 [3, u_stride] with u_stride >= draft_len + 1 = 3, not (4, 6)',
    'spec/u-stride': 'spec_advance: u must be f32 [3, u_stride] with u_stride >= draft_len + 1 = 3, not (3, 0)',
    'spec/block_table-dtype': 'spec_advance: block_table must be int32 [3, blocks per row >= 1], not (3, 2)',
    'spec/block_table-rank': 'spec_advance: block_table must be int32 [3, blocks per row >= 1], not (2,)',
    'spec/block_table-rows': 'spec_advance: block_table must be int32 [3, blocks per row >= 1], not (2, 2)',
    'spec/block_table-width': 'spec_advance: block_table must be int32 [3, blocks per row >= 1], not (3, 0)',
    'spec/block_size-24': 'spec_advance: block_size must be a power of two in [16, 256], not 24',
    'spec/block_size-8': 'spec_advance: block_size must be a power of two in [16, 256], not 8',
    'spec/block_size-512': 'spec_advance: block_size must be a power of two in [16, 256], not 512',
    'spec/vocab-0': 'spec_advance: logits (9, 0) outside 1 <= vocab <= 262144, rows * (draft_len + 1) <= 65535',
    'spec/tick-dtype': 'spec_advance: tick must be int32 [3], not float64 (3,)',
    'spec/tick-rank': 'spec_advance: tick must be int32 [3], not int32 (3, 1)',
    'spec/tick-rows': 'spec_advance: tick must be int32 [3], not int32 (4,)',
    'spec/start-dtype': 'spec_advance: start must be int64 [3], not float64 (3,)',
    'spec/start-rank': 'spec_advance: start must be int64 [3], not int64 (3, 1)',
    'spec/start-rows': 'spec_advance: start must be int64 [3], not int64 (4,)',
    'spec/remaining-dtype': 'spec_advance: remaining must be int32 [3], not float64 (3,)',
    'spec/remaining-rank': 'spec_advance: remaining must be int32 [3], not int32 (3, 1)',
    'spec/remaining-rows': 'spec_advance: remaining must be int32 [3], not int32 (4,)',
    'spec/eos-dtype': 'spec_advance: eos must be int32 [3], not float64 (3,)',
    'spec/eos-rank': 'spec_advance: eos must be int32 [3], not int32 (3, 1)',
    'spec/eos-rows': 'spec_advance: eos must be int32 [3], not int32 (4,)',
    'spec/hist_len-dtype': 'spec_advance: hist_len must be int32 [3], not float64 (3,)',
    'spec/hist_len-rank': 'spec_advance: hist_len must be int32 [3], not int32 (3, 1)',
    'spec/hist_len-rows': 'spec_advance: hist_len must be int32 [3], not int32 (4,)',
    'spec/n_out-dtype': 'spec_advance: n_out must be int32 [3], not float64 (3,)',
    'spec/n_out-rank': 'spec_advance: n_out must be int32 [3], not int32 (3, 1)',
    'spec/n_out-rows': 'spec_advance: n_out must be int32 [3], not int32 (4,)',
    'spec/n_acc-dtype': 'spec_advance: n_acc must be int32 [3], not float64 (3,)',
    'spec/n_acc-rank': 'spec_advance: n_acc must be int32 [3], not int32 (3, 1)',
    'spec/n_acc-rows': 'spec_advance: n_acc must be int32 [3], not int32 (4,)',
    'spec/ids-dtype': 'spec_advance: ids must be int64 [rows, draft_len + 1] with 1 <= draft_len <= 15, not int32 (3, 3)',
    'spec/ids-rank': 'spec_advance: ids must be int64 [rows, draft_len + 1] with 1 <= draft_len <= 15, not int64 (3,)',
    'spec/ids-group-1': 'spec_advance: ids must be int64 [rows, draft_len + 1] with 1 <= draft_len <= 15, not int64 (3, 1)',
    'spec/ids-group-17': 'spec_advance: ids must be int64 [rows, draft_len + 1] with 1 <= draft_len <= 15, not int64 (3, 17)',
    'spec/logits-rows': 'spec_advance: logits hold 8 rows, ids (3, 3) asks for 9',
    'spec/u-short': 'spec_advance: u must be f32 [3, u_stride] with u_stride >= draft_len + 1 = 3, not (3, 2)',
    'spec/pos-dtype': 'spec_advance: pos must be int64 [3, 3], not int32 (3, 3)',
    'spec/pos-shape': 'spec_advance: pos must be int64 [3, 3], not int64 (3, 2)',
    'spec/slots-dtype': 'spec_advance: slots must be int64 [3, 3], not int32 (3, 3)',
    'spec/slots-shape': 'spec_advance: slots must be int64 [3, 3], not int64 (2, 3)',
    'spec/hist-dtype': 'spec_advance: hist must be int32 [3, hist_stride >= 1], not int64 (3, 9)',
    'spec/hist-rank': 'spec_advance: hist must be int32 [3, hist_stride >= 1], not int32 (9,)',
    'spec/hist-rows': 'spec_advance: hist must be int32 [3, hist_stride >= 1], not int32 (2, 9)',
    'spec/hist-width': 'spec_advance: hist must be int32 [3, hist_stride >= 1], not int32 (3, 0)',
    'spec/ngram_max-0': 'spec_advance: ngram_max must be in [1, 4], not 0',
    'spec/ngram_max-5': 'spec_advance: ngram_max must be in [1, 4], not 5',
    'spec/vocab-262145': 'spec_advance: logits (2, 262145) outside 1 <= vocab <= 262144, rows * (draft_len + 1) <= 65535',
    'spec/rows-65536': 'spec_advance: logits (65536, 8) outside 1 <= vocab <= 262144, rows * (draft_len + 1) <= 65535',
    'logprobs/logits-dtype': 'token_logprobs: logits must be fp16 [rows, vocab]',
    'logprobs/logits-rank': 'token_logprobs: logits must be fp16 [rows, vocab]',
    'logprobs/targets-dtype': 'token_logprobs: targets must be int64 [3], one entry per row, not int32 (3,)',
    'logprobs/targets-rank': 'token_logprobs: targets must be int64 [3], one entry per row, not int64 (3, 1)',
    'logprobs/targets-rows': 'token_logprobs: targets must be int64 [3], one entry per row, not int64 (2,)',
    'logprobs/vocab-0': 'token_logprobs: logits (3, 0) outside 1 <= vocab <= 262144, rows <= 1048576',
    'logprobs/vocab-262145': 'token_logprobs: logits (1, 262145) outside 1 <= vocab <= 262144, rows <= 1048576',
    'logprobs/rows-1048577': 'token_logprobs: logits (1048577, 8) outside 1 <= vocab <= 262144, rows <= 1048576',
    'sample_tokens/no-tensor': 'sample_tokens: logits must be an fp16 [rows, vocab] tensor and u an f32 [rows] tensor',
    'sample_tokens/u-no-tensor': 'sample_tokens: logits must be an fp16 [rows, vocab] tensor and u an f32 [rows] tensor',
    'sample_tokens/logits-rank': 'sample_tokens: logits must be an fp16 [rows, vocab] tensor and u an f32 [rows] tensor',
    'sample_tokens/temperature-count': 'sample_tokens: temperature holds 2 entries, the logits have 3 rows',
    'sample_tokens/top_k-count': 'sample_tokens: top_k holds 2 entries, the logits have 3 rows',
    'sample_tokens/top_p-device': "sample_tokens: top_p must be on the logits' device",
    'sample_advance/no-tensor': 'sample_advance: logits must be an fp16 [rows, vocab] tensor and u an f32 [rows, u_stride] tensor',
    'sample_advance/u-no-tensor': 'sample_advance: logits must be an fp16 [rows, vocab] tensor and u an f32 [rows, u_stride] tensor',
    'sample_advance/logits-rank': 'sample_advance: logits must be an fp16 [rows, vocab] tensor and u an f32 [rows, u_stride] tensor',
    'sample_advance/temperature-count': 'sample_advance: temperature holds 2 entries, the logits have 3 rows',
    'sample_advance/top_k-count': 'sample_advance: top_k holds 2 entries, the logits have 3 rows',
    'sample_advance/top_p-device': "sample_advance: top_p must be on the logits' device",
    'spec_advance/no-tensor': 'spec_advance: logits must be an fp16 [rows * (draft_len + 1), vocab] tensor, u an f32 [rows, u_stride] tensor and ids an int64 [rows, draft_len + 1] tensor',
    'spec_advance/u-no-tensor': 'spec_advance: logits must be an fp16 [rows * (draft_len + 1), vocab] tensor, u an f32 [rows, u_stride] tensor and ids an int64 [rows, draft_len + 1] tensor',
    'spec_advance/logits-rank': 'spec_advance: logits must be an fp16 [rows * (draft_len + 1), vocab] tensor, u an f32 [rows, u_stride] tensor and ids an int64 [rows, draft_len + 1] tensor',
    'spec_advance/temperature-count': 'spec_advance: temperature holds 2 entries, the logits have 9 rows',
    'spec_advance/top_k-count': 'spec_advance: top_k holds 2 entries, the logits have 9 rows',
    'spec_advance/top_p-device': "spec_advance: top_p must be on the logits' device",
    'spec_advance/ids-no-tensor': 'spec_advance: logits must be an fp16 [rows * (draft_len + 1), vocab] tensor, u an f32 [rows, u_stride] tensor and ids an int64 [rows, draft_len + 1] tensor',
    'token_logprobs/no-tensor': 'token_logprobs: logits must be an fp16 [rows, vocab] tensor and targets an int64 [rows] tensor',
    'token_logprobs/logits-rank': 'token_logprobs: logits must be an fp16 [rows, vocab] tensor and targets an int64 [rows] tensor',
    'cpu/rope_qkv': 'rope_qkv: every tensor must be on the GPU (there is no CPU path)',
    'cpu/decode_attention': 'decode_attention: every tensor must be on the GPU (there is no CPU path)',
    'cpu/rope_qkv_kv8': 'rope_qkv_kv8: every tensor must be on the GPU (there is no CPU path)',
    'cpu/decode_attention_kv8': 'decode_attention_kv8: every tensor must be on the GPU (there is no CPU path)',
    'cpu/rope_qkv_paged': 'rope_qkv_paged: every tensor must be on the GPU (there is no CPU path)',
    'cpu/rope_qkv_paged_kv8': 'rope_qkv_paged_kv8: every tensor must be on the GPU (there is no CPU path)',
    'cpu/decode_attention_paged': 'decode_attention_paged: every tensor must be on the GPU (there is no CPU path)',
    'cpu/decode_attention_paged_kv8': 'decode_attention_paged_kv8: every tensor must be on the GPU (there is no CPU path)',
    'cpu/prefill_attention_paged': 'prefill_attention_paged: every tensor must be on the GPU (there is no CPU path)',
    'cpu/prefill_attention_paged_kv8': 'prefill_attention_paged_kv8: every tensor must be on the GPU (there is no CPU path)',
    'cpu/sample_tokens': 'sample_tokens: every tensor must be on the GPU (there is no CPU path)',
    'cpu/sample_advance': 'sample_advance: every tensor must be on the GPU (there is no CPU path)',
    'cpu/spec_advance': 'spec_advance: every tensor must be on the GPU (there is no CPU path)',
    'cpu/token_logprobs': 'token_logprobs: logits and targets must be on the GPU (there is no CPU path)',
}


def test_table_and_cases_name_the_same_checks():
    ids = [cid for cid, _, _ in _cases()]
    assert len(set(ids)) == len(ids) and set(ids) == set(MESSAGES)
    assert sum(1 for m in MESSAGES.values() if m.endswith("every tensor must be on the GPU (there is no CPU path)")) == 13


@pytest.mark.parametrize("cid", list(MESSAGES))
def test_message_is_the_recorded_one(cid):
    fn, kwargs = next((f, kw) for c, f, kw in _cases() if c == cid)
    assert _message(fn, kwargs) == MESSAGES[cid]


if __name__ == "__main__":
    if sys.argv[1:] != ["--print"]:
        sys.exit(__doc__)
    print("MESSAGES = {")
    for cid, fn, kwargs in _cases():
        print(f"    {cid!r}: {_message(fn, kwargs)!r},")
    print("}")
