"""The shared-prefix decode attention without a GPU (include/qqq_amd_shared.h): the header and the exports, the argument checks of the two
entry points with fake aligned addresses (every refusal happens before any launch), the plan entry point against the decode plan's rule,
the kernels' entries in the gfx950 code object, the ops' fake shapes, the routing of fuse_shared() with host stubs for the ops, and what
the loops and generate() refuse."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 17
ENTRIES = {"qqq_decode_attn_paged_shared", "qqq_decode_attn_paged_shared_kv8", "qqq_decode_attn_shared_plan"}


@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def test_header_declares_the_three_functions_and_the_library_exports_them(L):
    from qqq_amd import _abi

    names = set(_abi.prototypes(os.path.join(ROOT, "include", "qqq_amd_shared.h")))
    assert names == ENTRIES
    for n in names:
        assert hasattr(L, n), n
    assert L.qqq_amd_abi_version() == 4  # symbols were only added (a change of the header rebuilds the library: tests/test_abi_cpu.py)


# fake device addresses with the alignment the entry points ask for: the calls below must fail in the checks, before any launch
A16, A8, A4 = 0x10000, 0x20008, 0x30004
WS = 1 << 30


def _call(L, kv8, q=A16, kp=A16, vp=A16, ks=A4, vs=A4, table=A4, stride=32, pos=A8, family=A4, shared=A8, pack=4, scale=0.088, o=A16, xq=A8,
          s1=A4, ws=A16, wsb=WS, b=8, h=32, kvh=8, d=128, nb=64, bs=128, max_len=4096):
    tail = (table, stride, pos, family, shared, pack, scale, o, xq, s1, ws, wsb, b, h, kvh, d, nb, bs, max_len, 0, None)
    return L.qqq_decode_attn_paged_shared_kv8(q, kp, vp, ks, vs, *tail) if kv8 else L.qqq_decode_attn_paged_shared(q, kp, vp, *tail)


# DEC_BAD of tests/test_paged_cpu.py, the two descriptors and the pack's own limits
BAD = [dict(q=None), dict(kp=None), dict(vp=None), dict(table=None), dict(pos=None), dict(ws=None), dict(o=None, xq=None, s1=None),
       dict(xq=None), dict(s1=None), dict(d=96), dict(d=256), dict(d=32), dict(h=72), dict(h=30), dict(h=0), dict(kvh=0),
       dict(h=256, kvh=32), dict(q=A16 + 8), dict(kp=A16 + 2), dict(vp=A16 + 4), dict(table=A4 + 2), dict(table=A4 + 1), dict(pos=A8 + 4),
       dict(o=A16 + 8), dict(xq=A8 + 4), dict(s1=A4 + 2), dict(ws=A16 + 8), dict(wsb=0), dict(wsb=1000), dict(max_len=0), dict(max_len=-1),
       dict(max_len=4097), dict(stride=31), dict(stride=0, max_len=1), dict(stride=-1), dict(b=-1), dict(b=65536), dict(bs=8, stride=512),
       dict(bs=24, stride=512), dict(bs=512, stride=512), dict(nb=0), dict(nb=-1), dict(nb=1 << 24, bs=256),
       dict(family=None), dict(shared=None), dict(family=A4 + 2), dict(family=A4 + 1), dict(shared=A8 + 4), dict(shared=A8 + 1),
       dict(pack=0), dict(pack=-1), dict(pack=17), dict(pack=65), dict(h=64, kvh=8, pack=9), dict(h=8, kvh=8, pack=65),
       # pack = 1 is the plain call, and refused like it
       dict(pack=1, q=None), dict(pack=1, family=None), dict(pack=1, shared=A8 + 4), dict(pack=1, wsb=0), dict(pack=1, d=96)]
BAD_KV8 = [dict(ks=None), dict(vs=None), dict(ks=A4 + 2), dict(vs=A4 + 1), dict(pack=1, ks=None)]


@pytest.mark.parametrize("kv8,kw", [(False, kw) for kw in BAD] + [(True, kw) for kw in BAD + BAD_KV8])
def test_shared_attn_rejects_bad_arguments(L, kv8, kw):
    from qqq_amd import _lib

    assert _call(L, kv8, **kw) == ERR_ARG
    assert _lib.last_error().startswith("qqq_decode_attn_paged_shared_kv8:" if kv8 else "qqq_decode_attn_paged_shared:")


def test_the_refused_packs_are_the_ones_meant(L):
    assert (32 // 8) * 17 == 68 > 64 == (32 // 8) * 16 and (64 // 8) * 9 == 72
    assert _call(L, False, b=0) == 0 and _call(L, True, b=0, q=None) == 0  # b = 0 is a no-op


def _plan(L, b, h, kvh, max_len, pack):
    splits, chunk = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.qqq_decode_attn_shared_plan(b, h, kvh, max_len, pack, ctypes.byref(splits), ctypes.byref(chunk))
    return rc, splits.value, chunk.value


@pytest.mark.parametrize("b,h,kvh,max_len,pack", [(1, 32, 32, 1, 1), (8, 32, 8, 4096, 4), (24, 8, 2, 1024, 8), (3, 28, 4, 1000, 2),
                                                  (64, 32, 8, 16384 + 37, 8), (256, 64, 8, 131072, 2), (16, 32, 32, 640, 64)])
def test_plan_is_the_decode_plan(L, b, h, kvh, max_len, pack):
    rc, splits, chunk = _plan(L, b, h, kvh, max_len, pack)
    assert rc == 0
    assert chunk > 0 and chunk % 128 == 0 and splits == -(-max_len // chunk)
    # the rule of qqq_decode_attn: about four workgroups per compute unit (256 where there is no device), at most 32 splits and no
    # fewer than 128 keys per split
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    want = max(1, min(-(-4 * cus // (b * kvh)), min(32, -(-max_len // 128))))
    assert chunk == -(-(-(-max_len // want)) // 128) * 128
    assert splits * (b * h * (128 + 2) * 4) <= L.qqq_decode_attn_workspace_bytes(b, h, kvh, 128, max_len)  # the workspace covers the plan


@pytest.mark.parametrize("kw", [dict(b=0), dict(b=-1), dict(b=65536), dict(h=30), dict(h=72), dict(kvh=0), dict(max_len=0), dict(pack=0),
                                dict(pack=17), dict(pack=-3)])
def test_plan_refuses_what_the_entry_points_refuse(L, kw):
    from qqq_amd import _lib

    args = dict(b=8, h=32, kvh=8, max_len=4096, pack=4)
    args.update(kw)
    assert _plan(L, **args)[0] == ERR_ARG
    assert _lib.last_error().startswith("qqq_decode_attn_shared_plan:")
    assert L.qqq_decode_attn_shared_plan(8, 32, 8, 4096, 4, None, None) == ERR_ARG


def test_kernels_are_in_the_code_object_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    from qqq_amd import build

    table = {k["demangled"]: k for k in code_object.kernels(build.LIB)}
    for fam in ("qqq_shared_split_kernel", "qqq_shared_kv8_split_kernel"):
        for d in (64, 128):
            for nq in (1, 2, 4):
                k = table[f"{fam}<{d},{nq}>"]
                assert not k["private_segment_fixed_size"] and not k["vgpr_spill_count"] and not k["sgpr_spill_count"], (fam, d, nq, k)


def _attn(h=8, kvh=2, d=64):
    from qqq_amd.attention import QuantLlamaAttention

    return QuantLlamaAttention(h * d, h, kvh, head_dim=d, group_size=-1, layer_idx=0)


def test_fuse_shared_flags_follow_fuse_verify():
    from qqq_amd.attention import QuantLlamaDecoderLayer
    from qqq_amd.model import QuantLlamaForCausalLM, QuantLlamaModel

    attn = _attn()
    assert not attn.shared_fused and attn.fuse_shared() is attn and attn.shared_fused
    assert attn.unfuse_shared() is attn and not attn.shared_fused
    assert "_shared" not in attn.state_dict()
    for cls in (QuantLlamaDecoderLayer, QuantLlamaModel, QuantLlamaForCausalLM):
        for name in ("fuse_shared", "unfuse_shared", "shared_fused"):
            assert hasattr(cls, name), (cls, name)


def test_loops_and_generate_refuse_what_they_cannot_serve():
    from qqq_amd.model import QuantLlamaForCausalLM
    from qqq_amd.paged import PagedKVCache
    from qqq_amd.serve import DecodeLoop, SpecDecodeLoop

    class LM:  # the constructors look at the head's device before anything else
        lm_head = torch.nn.Linear(4, 4)

    cache = PagedKVCache(1, 8, 2, 64, 16, device="cpu")
    with pytest.raises(ValueError, match="family"):
        DecodeLoop(LM(), cache, rows=6, max_len=64, graph=False, family=4)
    with pytest.raises(ValueError, match="family"):
        DecodeLoop(LM(), cache, rows=4, max_len=64, graph=False, family=0)
    with pytest.raises(ValueError, match="family"):
        SpecDecodeLoop(LM(), cache, rows=4, max_len=64, draft_len=2, graph=False, family=2)
    gen = QuantLlamaForCausalLM.generate
    with pytest.raises(ValueError, match="n=0"):
        gen(None, [[1, 2]], 4, n=0)
    with pytest.raises(ValueError, match="draft_len"):
        gen(None, [[1, 2]], 4, n=2, draft_len=2, device_loop=True)
