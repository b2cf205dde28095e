"""Operator layer: the reference's `qqq_gemm` signature on top of the C-ABI (include/qqq_amd.h).

`qqq_gemm` is positionally identical to `QQQ._CUDA.qqq_gemm` (csrc/pybind.cpp:3-5,
csrc/qqq_gemm.cu:1048-1106, qqq_gemm.h:23-36) and raises RuntimeError in the same situations with
the same messages.  It is also registered as the torch custom op `qqq_amd::qqq_gemm`
(torch.library), so it does not graph-break under torch.compile.
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib

ERR_PROB_SHAPE = 1
ERR_KERN_SHAPE = 2
_FORCE_DISPATCHER = os.environ.get("QQQ_AMD_FORCE_DISPATCHER", "0") == "1"


def _load_torch_ext():
    """The compiled binding (csrc/qqq_torch.cpp -> qqq_amd/_torch_ext*.so): the eager fast path -- same C-ABI calls, same checks
    and messages, ~2 us of host time per call instead of ~7.5 through ctypes.  Absent (not built) -> the ctypes binding below
    serves; both end in libqqq_amd.so.  Not used with a QQQ_AMD_LIB override (the module binds the default library)."""
    if os.environ.get("QQQ_AMD_LIB") or os.environ.get("QQQ_AMD_NO_TORCH_EXT") == "1":
        return None
    try:
        _lib.lib()  # the operator library first: the module's NEEDED entry then resolves to the same mapping
        from . import _torch_ext  # type: ignore

        return _torch_ext if _torch_ext.abi_version() == _lib.ABI_VERSION else None
    except Exception:
        return None


_EXT = None
_EXT_TRIED = False


def _ext():
    global _EXT, _EXT_TRIED
    if not _EXT_TRIED:
        _EXT_TRIED = True
        _EXT = _load_torch_ext()
    return _EXT


def _ptr(t: Optional[torch.Tensor]):
    # plain ints: the argtypes declared in _lib.py convert them to void* (cheaper than building c_void_p objects)
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_for(t: torch.Tensor):
    # the raw hipStream_t of t's device; the private fast path saves ~1.5 us of Stream-object construction per call
    if _raw_stream is not None:
        idx = t.device.index
        return _raw_stream(idx if idx is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


def _dt(dtype) -> str:
    return str(dtype).replace("torch.", "")


def _same_gpu(name, ts):
    # every tensor of `ts` on the GPU, and on the GPU of the first
    if not all(t.is_cuda for t in ts):
        raise RuntimeError(f"{name}: every tensor must be on the GPU (there is no CPU path)")
    if any(t.device != ts[0].device for t in ts):
        raise RuntimeError(f"{name}: every tensor must be on the same GPU")


def _raise_lib(name, err):
    # the library's own refusal of a call: its error code and message, under the op's name (None: the GEMM entry points, _raise_for)
    if err:
        raise RuntimeError(f"qqq_amd: {name + ' ' if name else ''}error {err}: {_lib.last_error()}")


def _check_common(A, B, C, D, s1, s2, s3, workspace, max_par):
    # the reference's own checks (csrc/qqq_gemm.cu:1062-1075) ...
    prob_m, prob_n, prob_k = A.size(0), C.size(1), A.size(1)
    groupsize = -1 if s3.numel() == 0 else prob_k // s3.size(0)
    if groupsize != -1 and groupsize * s3.size(0) != prob_k:
        raise RuntimeError(f"k={prob_k} not compatible with {s3.size(0)} groups.")
    if workspace.numel() < prob_n // 128 * max_par:
        raise RuntimeError(f"workspace must be of size at least {prob_n // 128 * max_par}.")
    if s1.dtype != torch.float32:
        raise RuntimeError(f"s1 dtype must be float32, but got {s1.dtype}.")
    if s2.dtype != torch.float32:
        raise RuntimeError(f"s2 dtype must be float32, but got {s2.dtype}.")
    if s3.dtype != torch.float16:
        raise RuntimeError(f"s3 dtype must be float16, but got {s3.dtype}.")
    # ... plus the ones the reference leaves as undefined behaviour (SURVEY 8b "Errors")
    if A.dtype != torch.int8 or B.dtype != torch.int32 or D.dtype != torch.float16 or C.dtype != torch.int32:
        raise RuntimeError("qqq_gemm: expected A int8, B int32, C int32, D float16")
    if workspace.dtype != torch.int32:
        raise RuntimeError("qqq_gemm: workspace must be int32")
    for name, t in (("A", A), ("B", B), ("C", C), ("D", D), ("s1", s1), ("s2", s2), ("workspace", workspace)):
        if not t.is_contiguous():
            raise RuntimeError(f"qqq_gemm: {name} must be contiguous")
        if not t.is_cuda or t.device != A.device:
            raise RuntimeError(f"qqq_gemm: {name} must live on the same GPU as A (there is no CPU path)")
    if s3.numel() and (not s3.is_contiguous() or s3.device != A.device):
        raise RuntimeError("qqq_gemm: s3 must be contiguous and on A's device")
    if B.numel() != (prob_k // 16) * (prob_n * 2) or D.numel() != prob_m * prob_n:
        raise RuntimeError("qqq_gemm: B must be [k/16, 2n] and D [m, n]")
    if s1.numel() != prob_m or s2.numel() != prob_n:
        raise RuntimeError("qqq_gemm: s1 must have m and s2 n elements")
    if C.size(0) < max_par * 64:
        raise RuntimeError(f"qqq_gemm: C must have at least max_par*64={max_par * 64} rows")
    return prob_m, prob_n, prob_k, groupsize


def _raise_for(err, prob_m, prob_n, prob_k, thread_k, thread_n, groupsize):
    if err == 0:
        return
    if err == ERR_PROB_SHAPE:  # csrc/qqq_gemm.cu:1096-1100
        raise RuntimeError(
            f"Problem (m={prob_m}, n={prob_n}, k={prob_k}) not compatible with thread_k={thread_k}, thread_n={thread_n}."
        )
    if err == ERR_KERN_SHAPE:  # csrc/qqq_gemm.cu:1101-1105
        raise RuntimeError(
            f"No kernel implementation for thread_k={thread_k}, thread_n={thread_n}, groupsize={groupsize}."
        )
    _raise_lib(None, err)


def _check_w8(W8, prob_k, prob_n, groupsize, device):
    if W8 is None or W8.numel() == 0:
        return None
    if (W8.dtype != torch.int8 or W8.numel() != prob_k * prob_n or not W8.is_contiguous() or W8.device != device
            or groupsize not in (128, -1)):
        raise RuntimeError("W8 must be the contiguous int8 [k * n] tensor of expand_int8 on A's device")
    return W8


def qqq_gemm_ex(A, B, C, D, s1, s2, s3, workspace, thread_k=-1, thread_n=-1, sms=-1, max_par=8,
                tune: Optional[dict] = None, acc_out: Optional[torch.Tensor] = None,
                bias: Optional[torch.Tensor] = None, W8: Optional[torch.Tensor] = None) -> None:
    """qqq_gemm with tuning / debug hooks (tests, bench), the fused fp16 bias epilogue and (per-group layers, opt-in) the
    layer's expanded int8 weights `W8` (expand_int8; used where the plan is the wide kernel's, bit-identical results).
    `tune` keys: kernel, ksplit, waves, fused, bm, glds, pf, stages, mt, pw, split_m, skew, w8 (include/qqq_amd.h)."""
    L = _lib.lib()
    prob_m, prob_n, prob_k, groupsize = _check_common(A, B, C, D, s1, s2, s3, workspace, max_par)
    tn = None
    if tune:
        tn = _lib.QQQTune()
        for k, v in tune.items():
            setattr(tn, k, int(v))
    if acc_out is not None:
        if acc_out.dtype != torch.int32 or acc_out.numel() != prob_m * prob_n or not acc_out.is_contiguous():
            raise RuntimeError("acc_out must be a contiguous int32 [m, n] tensor")
    if bias is not None:
        if bias.dtype != torch.float16 or bias.numel() != prob_n or not bias.is_contiguous() or bias.device != A.device:
            raise RuntimeError("bias must be a contiguous fp16 [n] tensor on A's device")
    W8 = _check_w8(W8, prob_k, prob_n, groupsize, A.device)
    err = L.qqq_w4a8_gemm_ex2(
        _ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(s1), _ptr(s2), _ptr(s3), prob_m, prob_n, prob_k,
        _ptr(workspace), groupsize, A.device.index if A.device.index is not None else 0, _stream_for(A),
        thread_k, thread_n, sms, max_par, ctypes.byref(tn) if tn is not None else None, _ptr(acc_out),
        _ptr(bias), _ptr(W8),
    )
    _raise_for(err, prob_m, prob_n, prob_k, thread_k, thread_n, groupsize)


def _qqq_gemm_impl(A, B, C, D, s1, s2, s3, workspace, thread_k, thread_n, sms, max_par) -> None:
    L = _lib.lib()
    prob_m, prob_n, prob_k, groupsize = _check_common(A, B, C, D, s1, s2, s3, workspace, max_par)
    err = L.qqq_w4a8_gemm(
        _ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(s1), _ptr(s2), _ptr(s3), prob_m, prob_n, prob_k,
        _ptr(workspace), groupsize, A.device.index if A.device.index is not None else 0, _stream_for(A),
        thread_k, thread_n, sms, max_par,
    )
    _raise_for(err, prob_m, prob_n, prob_k, thread_k, thread_n, groupsize)


@torch.library.custom_op("qqq_amd::qqq_gemm", mutates_args=("C", "D", "workspace"))
def _qqq_gemm_op(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, D: torch.Tensor, s1: torch.Tensor,
                 s2: torch.Tensor, s3: torch.Tensor, workspace: torch.Tensor, thread_k: int, thread_n: int,
                 sms: int, max_par: int) -> None:
    _qqq_gemm_impl(A, B, C, D, s1, s2, s3, workspace, thread_k, thread_n, sms, max_par)


@torch.library.custom_op("qqq_amd::qqq_gemm_bias", mutates_args=("C", "D", "workspace"))
def _qqq_gemm_bias_op(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, D: torch.Tensor, s1: torch.Tensor,
                      s2: torch.Tensor, s3: torch.Tensor, workspace: torch.Tensor, bias: torch.Tensor,
                      max_par: int) -> None:
    qqq_gemm_ex(A, B, C, D, s1, s2, s3, workspace, -1, -1, -1, max_par, bias=bias)


@torch.library.custom_op("qqq_amd::qqq_gemm_w8", mutates_args=("C", "D", "workspace"))
def _qqq_gemm_w8_op(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, D: torch.Tensor, s1: torch.Tensor,
                    s2: torch.Tensor, s3: torch.Tensor, workspace: torch.Tensor, bias: Optional[torch.Tensor],
                    W8: Optional[torch.Tensor], max_par: int) -> None:
    qqq_gemm_ex(A, B, C, D, s1, s2, s3, workspace, -1, -1, -1, max_par, bias=bias, W8=W8)


def _expand_int8_impl(B: torch.Tensor, s_group: torch.Tensor) -> torch.Tensor:
    if B.dtype != torch.int32 or not B.is_cuda or not B.is_contiguous() or B.dim() != 2:
        raise RuntimeError("expand_int8: B must be the packed int32 [k/16, 2n] weight on the GPU (there is no CPU path)")
    k, n = B.size(0) * 16, B.size(1) // 2
    grouped = s_group.numel() != 0
    if grouped and (s_group.dtype != torch.float16 or not s_group.is_contiguous() or s_group.device != B.device or s_group.dim() != 2
                    or s_group.size(1) != n or s_group.size(0) * 128 != k):
        raise RuntimeError("expand_int8: s_group must be the contiguous fp16 [k/128, n] tensor of a per-group layer on B's device (or empty: per-channel)")
    W8 = torch.empty(k * n, dtype=torch.int8, device=B.device)
    err = _lib.lib().qqq_expand_int8(_ptr(B), _ptr(s_group), _ptr(W8), k, n, 128 if grouped else -1, B.device.index or 0, _stream_for(B))
    _raise_lib("expand_int8", err)
    return W8


@torch.library.custom_op("qqq_amd::expand_int8", mutates_args=())
def _expand_int8_op(B: torch.Tensor, s_group: torch.Tensor) -> torch.Tensor:
    return _expand_int8_impl(B, s_group)


@_expand_int8_op.register_fake
def _(B, s_group):
    return B.new_empty(B.shape[0] * 16 * (B.shape[1] // 2), dtype=torch.int8)


def expand_int8(B: torch.Tensor, s_group: torch.Tensor) -> torch.Tensor:
    """Opt-in load-time re-layout of a layer (beside QuantLinear.pack, qlinear_marlin.py:181-262): the int4 weights as
    the int8 operand the reference kernel forms inside its loop -- per-group re-quantised ONCE, bit for bit dequant_per_group
    (csrc/qqq_gemm.cu:167-210); per-channel (`s_group` empty) 16 * w4 (:146-151) -- stored in the wide kernel's MFMA operand order
    (include/qqq_amd.h: qqq_expand_int8).  Returns int8 [k * n]."""
    if _compiling(B, s_group):
        return _expand_int8_op(B, s_group)
    return _EXT.expand_int8(B, s_group) if _ext() is not None else _expand_int8_impl(B, s_group)


def qqq_gemm_w8(A, B, C, D, s1, s2, s3, workspace, bias=None, W8=None, max_par=16) -> None:
    """qqq_gemm with the optional fused bias and the optional expanded int8 weights of the layer (expand_int8)."""
    if _compiling(A, B, C, D, s1, s2, s3, workspace, bias, W8):
        _qqq_gemm_w8_op(A, B, C, D, s1, s2, s3, workspace, bias, W8, max_par)
    elif _ext() is not None:
        _EXT.qqq_gemm_w8(A, B, C, D, s1, s2, s3, workspace, bias, W8, max_par)
    else:
        qqq_gemm_ex(A, B, C, D, s1, s2, s3, workspace, -1, -1, -1, max_par, bias=bias, W8=W8)


_PLAIN = (torch.Tensor, torch.nn.Parameter)


def _compiling(*tensors) -> bool:
    # Under torch.compile / make_fx / FakeTensorMode / torch.export / any TorchDispatchMode, or with tensor
    # subclasses among the arguments, the calls must go through the registered custom ops (no graph break,
    # fake-tensor propagation, visible to dispatch-based tooling).  For plain eager tensors the dispatcher round
    # trip of a Python custom op costs ~9 us per call -- more than a decode GEMM on a 4096x4096 layer takes on
    # the GPU (tools/host_overhead.py) -- so those calls go straight to the ctypes binding.
    # QQQ_AMD_FORCE_DISPATCHER=1 forces the dispatcher path everywhere.
    if torch.compiler.is_compiling() or _FORCE_DISPATCHER or _dispatch_modes_active():
        return True
    for t in tensors:
        if t is not None and type(t) not in _PLAIN:
            return True
    return False


_len_dispatch_stack = getattr(torch._C, "_len_torch_dispatch_stack", None)  # private: absent -> always the dispatcher path


def _dispatch_modes_active() -> bool:
    return True if _len_dispatch_stack is None else _len_dispatch_stack() > 0


def qqq_gemm_bias(A, B, C, D, s1, s2, s3, workspace, bias, max_par=16) -> None:
    """qqq_gemm + the reference's `D + self.bias` (qlinear_marlin.py:287) fused into the epilogue."""
    if _compiling(A, B, C, D, s1, s2, s3, workspace, bias):
        _qqq_gemm_bias_op(A, B, C, D, s1, s2, s3, workspace, bias, max_par)
    elif _ext() is not None:
        _EXT.qqq_gemm_bias(A, B, C, D, s1, s2, s3, workspace, bias, max_par)
    else:
        qqq_gemm_ex(A, B, C, D, s1, s2, s3, workspace, -1, -1, -1, max_par, bias=bias)


def qqq_gemm(A, B, C, D, s1, s2, s3, workspace, thread_k=-1, thread_n=-1, sms=-1, max_par=8) -> None:
    """Drop-in for `QQQ._CUDA.qqq_gemm` (qqq_gemm.h:23-36): writes fp16 `D` in place, returns None."""
    if _compiling(A, B, C, D, s1, s2, s3, workspace):
        _qqq_gemm_op(A, B, C, D, s1, s2, s3, workspace, thread_k, thread_n, sms, max_par)
    elif _ext() is not None:
        _EXT.qqq_gemm(A, B, C, D, s1, s2, s3, workspace, thread_k, thread_n, sms, max_par)
    else:
        _qqq_gemm_impl(A, B, C, D, s1, s2, s3, workspace, thread_k, thread_n, sms, max_par)


def mul(A, B, C, D, s1, s2, s3, workspace, thread_k=-1, thread_n=-1, sms=-1, max_par=16):
    """Drop-in for qlinear_marlin.mul (qlinear_marlin.py:28-45)."""
    qqq_gemm(A, B, C, D, s1, s2, s3, workspace, thread_k, thread_n, sms, max_par)


def marlin_qqq_gemm(a, b_q_weight, s_tok, s_ch, s_group, workspace, size_m, size_n, size_k):
    """vLLM-style wrapper (`ops.marlin_qqq_gemm`, external to the reference tree): allocates the
    int32 reduce buffer and the fp16 output itself and returns the output."""
    max_par = 16
    C = torch.empty((max_par * 64, size_n), dtype=torch.int32, device=a.device)
    D = torch.empty((size_m, size_n), dtype=torch.float16, device=a.device)
    if s_group is None:
        s_group = torch.empty(0, dtype=torch.float16, device=a.device)
    qqq_gemm(a, b_q_weight, C, D, s_tok, s_ch, s_group, workspace, -1, -1, -1, max_par)
    return D


def _dynamic_quant_impl(x: torch.Tensor):
    L = _lib.lib()
    if x.dtype != torch.float16 or not x.is_cuda or x.dim() < 1:
        raise RuntimeError("dynamic_quant: expected an fp16 tensor on the GPU (there is no CPU path)")
    # any rank, like the reference method (max over the last dim with keepdim, qlinear_marlin.py:265-268)
    k = x.shape[-1]
    x2 = x.reshape(-1, k).contiguous()
    m = x2.shape[0]
    xq = torch.empty((m, k), dtype=torch.int8, device=x.device)
    s1 = torch.empty((m, 1), dtype=torch.float32, device=x.device)
    err = L.qqq_dynamic_quant(_ptr(x2), _ptr(xq), _ptr(s1), m, k, x.device.index or 0, _stream_for(x))
    _raise_lib("dynamic_quant", err)
    return xq.reshape(x.shape), s1.reshape(x.shape[:-1] + (1,))


@torch.library.custom_op("qqq_amd::dynamic_quant", mutates_args=())
def _dynamic_quant_op(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    return _dynamic_quant_impl(x)


@_dynamic_quant_op.register_fake
def _(x):
    return x.new_empty(x.shape, dtype=torch.int8), x.new_empty(x.shape[:-1] + (1,), dtype=torch.float32)


def dynamic_quant(x: torch.Tensor):
    """Fused replacement of QuantLinear.dynamic_quant (qlinear_marlin.py:265-268) for an fp16 tensor of any rank:
    (int8 x.shape, f32 x.shape[:-1] + (1,)).  Deviations from the reference expression: an all-zero row quantises to
    0 with scale 0 (reference: 0/0 = NaN -> int8, undefined), and the scale is the torch-GPU evaluation
    fp16(amax * (1/127)) (a CPU run of the reference differs by one fp16 ulp of the scale on a few rows)."""
    if _compiling(x):
        return _dynamic_quant_op(x)
    return _EXT.dynamic_quant(x) if _ext() is not None else _dynamic_quant_impl(x)


def quantlinear_forward(x: torch.Tensor, B, C, s2, s3, workspace, bias=None, max_par: int = 16, W8=None) -> torch.Tensor:
    """QuantLinear.forward (qlinear_marlin.py:270-288) for a 2-D fp16 input in ONE binding call: fused dynamic int8
    quantisation + W4A8 GEMM (+ fp16 bias).  The buffers are a module's own (qlinear.QuantLinear): only the cheap
    checks are made here.  Under torch.compile the two registered custom ops are used instead."""
    if _compiling(x, B, C, s2, s3, workspace, bias, W8):
        xq, s1 = _dynamic_quant_op(x)
        D = torch.empty((x.shape[0], C.size(1)), dtype=torch.float16, device=x.device)
        if W8 is not None:
            _qqq_gemm_w8_op(xq, B, C, D, s1, s2, s3, workspace, bias, W8, max_par)
        elif bias is not None:
            _qqq_gemm_bias_op(xq, B, C, D, s1, s2, s3, workspace, bias, max_par)
        else:
            _qqq_gemm_op(xq, B, C, D, s1, s2, s3, workspace, -1, -1, -1, max_par)
        return D
    if _ext() is not None:
        return _EXT.quantlinear_forward(x, B, C, s2, s3, workspace, bias, max_par, W8)
    if x.dtype != torch.float16 or not x.is_cuda or x.dim() != 2 or not x.is_contiguous():
        raise RuntimeError("quantlinear_forward: expected a contiguous 2-D fp16 tensor on the GPU (there is no CPU path)")
    m, k = x.shape
    n = C.size(1)
    dev = x.device
    if B.size(0) * 16 != k or B.device != dev:
        raise RuntimeError("quantlinear_forward: B must be the packed [k/16, 2n] weight on x's device")
    groupsize = -1 if s3.numel() == 0 else k // s3.size(0)
    # everything the kernels would read as raw bits
    if B.numel() != (k // 16) * (n * 2):
        raise RuntimeError("quantlinear_forward: B must be the packed [k/16, 2n] weight on x's device")
    if (B.dtype != torch.int32 or C.dtype != torch.int32 or workspace.dtype != torch.int32 or s2.dtype != torch.float32
            or C.device != dev or s2.device != dev or workspace.device != dev
            or not (B.is_contiguous() and C.is_contiguous() and s2.is_contiguous() and workspace.is_contiguous())):
        raise RuntimeError("quantlinear_forward: expected contiguous int32 B / C / workspace and float32 s2 on x's device")
    if s2.numel() != n or C.size(0) < max_par * 64 or workspace.numel() < n // 128 * max_par:
        raise RuntimeError(f"quantlinear_forward: s2 needs n={n} elements, C max_par*64={max_par * 64} rows, "
                           f"workspace at least {n // 128 * max_par} entries")
    if s3.numel() and (s3.dtype != torch.float16 or s3.device != dev or not s3.is_contiguous()
                       or groupsize * s3.size(0) != k or s3.numel() != s3.size(0) * n):
        raise RuntimeError("quantlinear_forward: s3 must be a contiguous fp16 [k/groupsize, n] tensor on x's device")
    if bias is not None and (bias.dtype != torch.float16 or bias.numel() != n or bias.device != dev
                             or not bias.is_contiguous()):
        raise RuntimeError(f"quantlinear_forward: bias must be a contiguous fp16 [n] tensor on x's device "
                           f"(got {bias.dtype}, {tuple(bias.shape)}, {bias.device})")
    xq = torch.empty((m, k), dtype=torch.int8, device=x.device)
    s1 = torch.empty((m, 1), dtype=torch.float32, device=x.device)
    D = torch.empty((m, n), dtype=torch.float16, device=x.device)
    if m == 0:
        return D
    W8 = _check_w8(W8, k, n, groupsize, dev)
    err = _lib.lib().qqq_quantlinear_forward2(
        x.data_ptr(), xq.data_ptr(), s1.data_ptr(), B.data_ptr(), C.data_ptr(), D.data_ptr(), s2.data_ptr(),
        _ptr(s3), m, n, k, workspace.data_ptr(), groupsize, x.device.index or 0, _stream_for(x), max_par, _ptr(bias), _ptr(W8))
    _raise_for(err, m, n, k, -1, -1, groupsize)
    return D


# ---- activation quantisers of a decoder block (include/qqq_amd_act.h): the fp16 activation in front of a QuantLinear and its per-token
# int8 quantisation in one launch; (xq, s1) are bit for bit dynamic_quant(y) of the activation y they compute.

def _rmsnorm_quant_impl(x, weight, eps, residual, return_y):
    if x.dtype != torch.float16 or not x.is_cuda or x.dim() < 1:
        raise RuntimeError("rmsnorm_quant: expected an fp16 tensor on the GPU (there is no CPU path)")
    k = x.shape[-1]
    if weight.dtype != torch.float16 or weight.device != x.device or weight.numel() != k:
        raise RuntimeError(f"rmsnorm_quant: weight must be an fp16 [{k}] tensor on x's device")
    if residual is not None and (residual.dtype != torch.float16 or residual.device != x.device or residual.shape != x.shape
                                 or not residual.is_contiguous()):
        raise RuntimeError("rmsnorm_quant: residual must be a contiguous fp16 tensor of x's shape on x's device (it is updated in place)")
    if x.numel() == 0:
        return (x.new_empty(x.shape, dtype=torch.int8), x.new_empty(x.shape[:-1] + (1,), dtype=torch.float32),
                x.new_empty(x.shape if return_y else (0,)))
    x2 = x.reshape(-1, k).contiguous()
    m = x2.shape[0]
    xq = torch.empty((m, k), dtype=torch.int8, device=x.device)
    s1 = torch.empty((m, 1), dtype=torch.float32, device=x.device)
    y = torch.empty((m, k) if return_y else (0,), dtype=torch.float16, device=x.device)
    err = _lib.lib().qqq_rmsnorm_quant(_ptr(x2), _ptr(residual), _ptr(weight.contiguous()), float(eps), _ptr(y), _ptr(xq), _ptr(s1), m, k,
                                       x.device.index or 0, _stream_for(x))
    _raise_lib("rmsnorm_quant", err)
    return xq.reshape(x.shape), s1.reshape(x.shape[:-1] + (1,)), (y.reshape(x.shape) if return_y else y)


@torch.library.custom_op("qqq_amd::rmsnorm_quant", mutates_args=("residual",))
def _rmsnorm_quant_op(x: torch.Tensor, weight: torch.Tensor, eps: float, residual: Optional[torch.Tensor],
                      return_y: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _rmsnorm_quant_impl(x, weight, eps, residual, return_y)


@_rmsnorm_quant_op.register_fake
def _(x, weight, eps, residual, return_y):
    return (x.new_empty(x.shape, dtype=torch.int8), x.new_empty(x.shape[:-1] + (1,), dtype=torch.float32),
            x.new_empty(x.shape if return_y else (0,), dtype=torch.float16))


def rmsnorm_quant(x: torch.Tensor, weight: torch.Tensor, eps: float, residual: Optional[torch.Tensor] = None, return_y: bool = False):
    """LlamaRMSNorm of an fp16 tensor (transformers' formula: fp32 norm, cast to fp16, times the fp16 weight) fused with the per-token int8
    quantisation of its output: (int8 x.shape, f32 x.shape[:-1] + (1,)), plus the fp16 output y with `return_y`.  With `residual` the
    input of the norm is fp16(residual + x), which is also written back into `residual` (the decoder's `residual = residual + h`)."""
    if _compiling(x, weight, residual):
        out = _rmsnorm_quant_op(x, weight, eps, residual, return_y)
    else:
        out = _rmsnorm_quant_impl(x, weight, eps, residual, return_y)
    return out if return_y else out[:2]


def _rows(t: torch.Tensor, i: int):
    # (rows [m, i], row stride): a view where the kernel can read it in place (unit column stride, row stride >= i and a multiple of 8,
    # 16-byte aligned base), a contiguous copy otherwise
    r = t.reshape(-1, i)
    ld = r.stride(0) if r.shape[0] > 1 else i
    if r.stride(1) != 1 or ld < i or ld % 8 or r.data_ptr() % 16:
        r, ld = r.contiguous(), i
    return r, ld


def _silu_mul_quant_impl(gate, up, return_y):
    if gate.dtype != torch.float16 or up.dtype != torch.float16 or not gate.is_cuda or up.device != gate.device or gate.dim() < 1:
        raise RuntimeError("silu_mul_quant: expected fp16 gate and up on the same GPU (there is no CPU path)")
    if gate.shape != up.shape:
        raise RuntimeError(f"silu_mul_quant: gate {tuple(gate.shape)} and up {tuple(up.shape)} must have the same shape")
    i = gate.shape[-1]
    if gate.numel() == 0:
        return (gate.new_empty(gate.shape, dtype=torch.int8), gate.new_empty(gate.shape[:-1] + (1,), dtype=torch.float32),
                gate.new_empty(gate.shape if return_y else (0,)))
    (g2, ld_g), (u2, ld_u) = _rows(gate, i), _rows(up, i)
    m = g2.shape[0]
    xq = torch.empty((m, i), dtype=torch.int8, device=gate.device)
    s1 = torch.empty((m, 1), dtype=torch.float32, device=gate.device)
    y = torch.empty((m, i) if return_y else (0,), dtype=torch.float16, device=gate.device)
    err = _lib.lib().qqq_silu_mul_quant(_ptr(g2), ld_g, _ptr(u2), ld_u, _ptr(y), _ptr(xq), _ptr(s1), m, i, gate.device.index or 0,
                                        _stream_for(gate))
    _raise_lib("silu_mul_quant", err)
    return xq.reshape(gate.shape), s1.reshape(gate.shape[:-1] + (1,)), (y.reshape(gate.shape) if return_y else y)


@torch.library.custom_op("qqq_amd::silu_mul_quant", mutates_args=())
def _silu_mul_quant_op(gate: torch.Tensor, up: torch.Tensor, return_y: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _silu_mul_quant_impl(gate, up, return_y)


@_silu_mul_quant_op.register_fake
def _(gate, up, return_y):
    return (gate.new_empty(gate.shape, dtype=torch.int8), gate.new_empty(gate.shape[:-1] + (1,), dtype=torch.float32),
            gate.new_empty(gate.shape if return_y else (0,), dtype=torch.float16))


def silu_mul_quant(gate: torch.Tensor, up: torch.Tensor, return_y: bool = False):
    """F.silu(gate) * up on fp16 fused with the per-token int8 quantisation of the product: (int8 gate.shape, f32 gate.shape[:-1] + (1,)),
    plus the fp16 product y with `return_y`.  gate / up may be strided views (e.g. the two halves of one fused gate|up output) as long as
    their rows are contiguous; they are read in place."""
    out = _silu_mul_quant_op(gate, up, return_y) if _compiling(gate, up) else _silu_mul_quant_impl(gate, up, return_y)
    return out if return_y else out[:2]


# ---- RoPE + KV-cache write of an attention block (include/qqq_amd_attn.h): q/k/v rows straight from the projection output, rotated q in
# scaled_dot_product_attention's layout, rotated k and plain v into a static cache, in one launch.

def _rope_qkv_shapes(q, k, v, cos, pos, k_cache):
    # (b, s, h, kvh, d, cap) from the tensors' shapes; raises for anything the kernel could not take
    if k_cache.dim() != 4:
        raise RuntimeError("rope_qkv: k_cache must be fp16 [b, kvh, cap, d]")
    b, kvh, cap, d = k_cache.shape
    m = pos.numel()
    if b == 0 or m % b:
        raise RuntimeError(f"rope_qkv: pos holds {m} positions, not a multiple of the cache's batch {b}")
    s = m // b
    if m == 0 or d == 0:
        return b, s, 0, kvh, d, cap
    if q.numel() % (m * d) or k.numel() != m * kvh * d or v.numel() != m * kvh * d:
        raise RuntimeError(f"rope_qkv: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} must hold {m} token rows of h*{d}, "
                           f"{kvh}*{d}, {kvh}*{d} elements")
    if cos.dim() != 2 or cos.shape[1] != d:
        raise RuntimeError(f"rope_qkv: cos / sin must be fp16 [table_len, {d}]")
    return b, s, q.numel() // (m * d), kvh, d, cap


def _rope_qkv_impl(q, k, v, cos, sin, pos, k_cache, v_cache):
    ts = (q, k, v, cos, sin, pos, k_cache, v_cache)
    _same_gpu("rope_qkv", ts)
    if any(t.dtype != torch.float16 for t in (q, k, v, cos, sin, k_cache, v_cache)) or pos.dtype != torch.int64:
        raise RuntimeError("rope_qkv: q, k, v, cos, sin and the caches must be fp16, pos int64")
    b, s, h, kvh, d, cap = _rope_qkv_shapes(q, k, v, cos, pos, k_cache)
    if v_cache.shape != k_cache.shape or sin.shape != cos.shape:
        raise RuntimeError("rope_qkv: v_cache must have k_cache's shape and sin cos's shape")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if not t.is_contiguous():
            raise RuntimeError(f"rope_qkv: {name} must be contiguous (it is written in place)")
    q_out = torch.empty((b, h, s, d), dtype=torch.float16, device=q.device)
    if q_out.numel() == 0:
        return q_out
    (q2, ld_q), (k2, ld_k), (v2, ld_v) = _rows(q, h * d), _rows(k, kvh * d), _rows(v, kvh * d)
    cos, sin, pos = cos.contiguous(), sin.contiguous(), pos.contiguous()
    err = _lib.lib().qqq_rope_qkv(_ptr(q2), ld_q, _ptr(k2), ld_k, _ptr(v2), ld_v, _ptr(cos), _ptr(sin), cos.shape[0], _ptr(pos),
                                  _ptr(q_out), _ptr(k_cache), _ptr(v_cache), b, s, h, kvh, d, cap, q.device.index or 0, _stream_for(q))
    _raise_lib("rope_qkv", err)
    return q_out


@torch.library.custom_op("qqq_amd::rope_qkv", mutates_args=("k_cache", "v_cache"))
def _rope_qkv_op(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor,
                 k_cache: torch.Tensor, v_cache: torch.Tensor) -> torch.Tensor:
    return _rope_qkv_impl(q, k, v, cos, sin, pos, k_cache, v_cache)


@_rope_qkv_op.register_fake
def _(q, k, v, cos, sin, pos, k_cache, v_cache):
    b, s, h, _, d, _ = _rope_qkv_shapes(q, k, v, cos, pos, k_cache)
    return q.new_empty((b, h, s, d), dtype=torch.float16)


def rope_qkv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor,
             k_cache: torch.Tensor, v_cache: torch.Tensor) -> torch.Tensor:
    """transformers' apply_rotary_pos_emb on fp16 q and k, bit for bit, plus the cache update, in one launch.

    q, k, v    fp16 token rows ([b*s, h*d] / [b*s, kvh*d], or [b, s, ...]); strided views such as the column ranges of one fused q|k|v
               output are read in place when their rows are contiguous, copied otherwise
    cos, sin   fp16 [table_len, d], indexed by position;  pos  int64 [b*s] positions in device memory (token bi*s + si)
    k_cache, v_cache  fp16 [b, kvh, cap, d], updated in place: rotated k and plain v of token (bi, si) go to slot pos[bi*s + si] of row bi
    Returns q_out fp16 [b, h, s, d], the rotated q in scaled_dot_product_attention's layout.  A token whose position is outside
    [0, min(cap, table_len)) writes nothing (its q_out rows are left uninitialised)."""
    if _compiling(q, k, v, cos, sin, pos, k_cache, v_cache):
        return _rope_qkv_op(q, k, v, cos, sin, pos, k_cache, v_cache)
    return _rope_qkv_impl(q, k, v, cos, sin, pos, k_cache, v_cache)


# ---- split-K decode attention (include/qqq_amd_decode.h): one query token per batch row over the static KV cache, written as o_proj's
# int8-quantised input; two launches (splits, then the combine that quantises).

def _decode_attention_shapes(q_out, k_cache, pos, max_len):
    # (b, h, kvh, d, cap, max_len) from the tensors' shapes; raises for anything the kernels could not take
    if k_cache.dim() != 4:
        raise RuntimeError("decode_attention: k_cache must be fp16 [b, kvh, cap, d]")
    b, kvh, cap, d = k_cache.shape
    if q_out.dim() != 4 or q_out.shape[0] != b or q_out.shape[2] != 1 or q_out.shape[3] != d:
        raise RuntimeError(f"decode_attention: q_out {tuple(q_out.shape)} must be [{b}, h, 1, {d}] (rope_qkv's output at s = 1)")
    if pos.numel() != b:
        raise RuntimeError(f"decode_attention: pos holds {pos.numel()} positions, the cache's batch is {b}")
    max_len = cap if max_len is None else int(max_len)
    return b, q_out.shape[1], kvh, d, cap, max_len


def _decode_attention_impl(q_out, k_cache, v_cache, pos, scale, max_len, return_fp16):
    ts = (q_out, k_cache, v_cache, pos)
    _same_gpu("decode_attention", ts)
    if any(t.dtype != torch.float16 for t in (q_out, k_cache, v_cache)) or pos.dtype != torch.int64:
        raise RuntimeError("decode_attention: q_out and the caches must be fp16, pos int64")
    b, h, kvh, d, cap, max_len = _decode_attention_shapes(q_out, k_cache, pos, max_len)
    if v_cache.shape != k_cache.shape:
        raise RuntimeError("decode_attention: v_cache must have k_cache's shape")
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise RuntimeError("decode_attention: the caches must be contiguous")
    dev = q_out.device
    xq = torch.empty((b, h * d), dtype=torch.int8, device=dev)
    s1 = torch.empty((b, 1), dtype=torch.float32, device=dev)
    o16 = torch.empty((b, h * d) if return_fp16 else (0,), dtype=torch.float16, device=dev)
    if b == 0:
        return xq, s1, o16
    L = _lib.lib()
    nbytes = L.qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len)
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)  # torch's allocator: also under stream / graph capture
    q2, pos = q_out.contiguous(), pos.contiguous()
    err = L.qqq_decode_attn(_ptr(q2), _ptr(k_cache), _ptr(v_cache), _ptr(pos), float(scale), _ptr(o16), _ptr(xq), _ptr(s1), _ptr(ws),
                            ws.numel(), b, h, kvh, d, cap, max_len, dev.index or 0, _stream_for(q_out))
    _raise_lib("decode_attention", err)
    return xq, s1, o16


@torch.library.custom_op("qqq_amd::decode_attn", mutates_args=())
def _decode_attn_op(q_out: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor, scale: float,
                    max_len: Optional[int], return_fp16: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _decode_attention_impl(q_out, k_cache, v_cache, pos, scale, max_len, return_fp16)


@_decode_attn_op.register_fake
def _(q_out, k_cache, v_cache, pos, scale, max_len, return_fp16):
    b, h, _, d, _, _ = _decode_attention_shapes(q_out, k_cache, pos, max_len)
    return (q_out.new_empty((b, h * d), dtype=torch.int8), q_out.new_empty((b, 1), dtype=torch.float32),
            q_out.new_empty((b, h * d) if return_fp16 else (0,), dtype=torch.float16))


def decode_attention(q_out: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor, scale: float,
                     max_len: Optional[int] = None, return_fp16: bool = False):
    """Attention of one query token per batch row over the static KV cache, quantised for o_proj: (xq int8 [b, h*d], s1 f32 [b, 1]) --
    dynamic_quant of the fp16 attention output, bit for bit -- plus that fp16 output [b, h*d] with `return_fp16`.

    q_out      fp16 [b, h, 1, d], rope_qkv's output at s = 1;  k_cache, v_cache  fp16 [b, kvh, cap, d] (h % kvh == 0, h / kvh <= 8,
               d 64 or 128, h*d <= 16384)
    pos        int64 [b] positions in device memory: row bi attends keys 0 ... pos[bi] (the new token already in the cache)
    scale      the score scale (head_dim ** -0.5);  max_len  the launch is sized for positions below it (default: cap), so a captured graph
               replays at any position below max_len
    Split-K over the keys with all query heads of a KV head in one workgroup; fp32 softmax and accumulation, probabilities rounded to fp16
    for the P.V product.  A row whose position is outside [0, min(cap, max_len)) writes nothing (its outputs are left uninitialised)."""
    if _compiling(q_out, k_cache, v_cache, pos):
        out = _decode_attn_op(q_out, k_cache, v_cache, pos, scale, max_len, return_fp16)
    else:
        out = _decode_attention_impl(q_out, k_cache, v_cache, pos, scale, max_len, return_fp16)
    return out if return_fp16 else out[:2]


# ---- the int8 KV cache (include/qqq_amd_kv8.h): rope_qkv and decode_attention over caches that hold every head row as dynamic_quant of
# the fp16 row -- int8 codes [b, kvh, cap, d] and one f32 scale per row [b, kvh, cap].

def _kv8_check_caches(name, k_cache, v_cache, k_scale, v_scale):
    if any(t.dtype != torch.int8 for t in (k_cache, v_cache)) or any(t.dtype != torch.float32 for t in (k_scale, v_scale)):
        raise RuntimeError(f"{name}: the caches must be int8 and their scales f32")
    if k_cache.dim() != 4:
        raise RuntimeError(f"{name}: k_cache must be int8 [b, kvh, cap, d]")
    if v_cache.shape != k_cache.shape or k_scale.shape != k_cache.shape[:3] or v_scale.shape != k_cache.shape[:3]:
        raise RuntimeError(f"{name}: v_cache must have k_cache's shape [b, kvh, cap, d] and the scales its first three dimensions")
    for nm, t in (("k_cache", k_cache), ("v_cache", v_cache), ("k_scale", k_scale), ("v_scale", v_scale)):
        if not t.is_contiguous():
            raise RuntimeError(f"{name}: {nm} must be contiguous")


def _rope_qkv_kv8_impl(q, k, v, cos, sin, pos, k_cache, v_cache, k_scale, v_scale):
    ts = (q, k, v, cos, sin, pos, k_cache, v_cache, k_scale, v_scale)
    _same_gpu("rope_qkv_kv8", ts)
    if any(t.dtype != torch.float16 for t in (q, k, v, cos, sin)) or pos.dtype != torch.int64:
        raise RuntimeError("rope_qkv_kv8: q, k, v, cos and sin must be fp16, pos int64")
    _kv8_check_caches("rope_qkv_kv8", k_cache, v_cache, k_scale, v_scale)
    b, s, h, kvh, d, cap = _rope_qkv_shapes(q, k, v, cos, pos, k_cache)
    if sin.shape != cos.shape:
        raise RuntimeError("rope_qkv_kv8: sin must have cos's shape")
    q_out = torch.empty((b, h, s, d), dtype=torch.float16, device=q.device)
    if q_out.numel() == 0:
        return q_out
    (q2, ld_q), (k2, ld_k), (v2, ld_v) = _rows(q, h * d), _rows(k, kvh * d), _rows(v, kvh * d)
    cos, sin, pos = cos.contiguous(), sin.contiguous(), pos.contiguous()
    err = _lib.lib().qqq_rope_qkv_kv8(_ptr(q2), ld_q, _ptr(k2), ld_k, _ptr(v2), ld_v, _ptr(cos), _ptr(sin), cos.shape[0], _ptr(pos),
                                      _ptr(q_out), _ptr(k_cache), _ptr(v_cache), _ptr(k_scale), _ptr(v_scale), b, s, h, kvh, d, cap,
                                      q.device.index or 0, _stream_for(q))
    _raise_lib("rope_qkv_kv8", err)
    return q_out


@torch.library.custom_op("qqq_amd::rope_qkv_kv8", mutates_args=("k_cache", "v_cache", "k_scale", "v_scale"))
def _rope_qkv_kv8_op(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor,
                     k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor) -> torch.Tensor:
    return _rope_qkv_kv8_impl(q, k, v, cos, sin, pos, k_cache, v_cache, k_scale, v_scale)


@_rope_qkv_kv8_op.register_fake
def _(q, k, v, cos, sin, pos, k_cache, v_cache, k_scale, v_scale):
    b, s, h, _, d, _ = _rope_qkv_shapes(q, k, v, cos, pos, k_cache)
    return q.new_empty((b, h, s, d), dtype=torch.float16)


def rope_qkv_kv8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor,
                 k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor) -> torch.Tensor:
    """rope_qkv into an int8 cache, one launch: q_out is rope_qkv's, bit for bit; the rotated k row and the plain v row of every (token,
    KV head) are stored as dynamic_quant of the fp16 row rope_qkv would have cached, bit for bit.

    q, k, v, cos, sin, pos   as for rope_qkv (head_dim 64 or 128)
    k_cache, v_cache  int8 [b, kvh, cap, d];  k_scale, v_scale  f32 [b, kvh, cap]; all four updated in place at each token's position
    Returns q_out fp16 [b, h, s, d].  A token whose position is outside [0, min(cap, table_len)) writes nothing."""
    ts = (q, k, v, cos, sin, pos, k_cache, v_cache, k_scale, v_scale)
    if _compiling(*ts):
        return _rope_qkv_kv8_op(*ts)
    return _rope_qkv_kv8_impl(*ts)


def _decode_attention_kv8_impl(q_out, k_cache, v_cache, k_scale, v_scale, pos, scale, max_len, return_fp16):
    ts = (q_out, k_cache, v_cache, k_scale, v_scale, pos)
    _same_gpu("decode_attention_kv8", ts)
    if q_out.dtype != torch.float16 or pos.dtype != torch.int64:
        raise RuntimeError("decode_attention_kv8: q_out must be fp16, pos int64")
    _kv8_check_caches("decode_attention_kv8", k_cache, v_cache, k_scale, v_scale)
    b, h, kvh, d, cap, max_len = _decode_attention_shapes(q_out, k_cache, pos, max_len)
    dev = q_out.device
    xq = torch.empty((b, h * d), dtype=torch.int8, device=dev)
    s1 = torch.empty((b, 1), dtype=torch.float32, device=dev)
    o16 = torch.empty((b, h * d) if return_fp16 else (0,), dtype=torch.float16, device=dev)
    if b == 0:
        return xq, s1, o16
    L = _lib.lib()
    nbytes = L.qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len)
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)  # torch's allocator: also under stream / graph capture
    q2, pos = q_out.contiguous(), pos.contiguous()
    err = L.qqq_decode_attn_kv8(_ptr(q2), _ptr(k_cache), _ptr(v_cache), _ptr(k_scale), _ptr(v_scale), _ptr(pos), float(scale), _ptr(o16),
                                _ptr(xq), _ptr(s1), _ptr(ws), ws.numel(), b, h, kvh, d, cap, max_len, dev.index or 0, _stream_for(q_out))
    _raise_lib("decode_attention_kv8", err)
    return xq, s1, o16


@torch.library.custom_op("qqq_amd::decode_attn_kv8", mutates_args=())
def _decode_attn_kv8_op(q_out: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                        pos: torch.Tensor, scale: float, max_len: Optional[int],
                        return_fp16: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _decode_attention_kv8_impl(q_out, k_cache, v_cache, k_scale, v_scale, pos, scale, max_len, return_fp16)


@_decode_attn_kv8_op.register_fake
def _(q_out, k_cache, v_cache, k_scale, v_scale, pos, scale, max_len, return_fp16):
    b, h, _, d, _, _ = _decode_attention_shapes(q_out, k_cache, pos, max_len)
    return (q_out.new_empty((b, h * d), dtype=torch.int8), q_out.new_empty((b, 1), dtype=torch.float32),
            q_out.new_empty((b, h * d) if return_fp16 else (0,), dtype=torch.float16))


def decode_attention_kv8(q_out: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                         pos: torch.Tensor, scale: float, max_len: Optional[int] = None, return_fp16: bool = False):
    """decode_attention over an int8 cache: (xq int8 [b, h*d], s1 f32 [b, 1]), plus the fp16 output [b, h*d] with `return_fp16`.

    q_out      fp16 [b, h, 1, d], rope_qkv_kv8's output at s = 1 (q is not quantised)
    k_cache, v_cache  int8 [b, kvh, cap, d];  k_scale, v_scale  f32 [b, kvh, cap]: the cache rope_qkv_kv8 fills, only read here
    pos, scale, max_len   as for decode_attention; so are the shape limits and the out-of-range rule
    Scores are (q . codes) in fp32 times k_scale[key] * scale; fp32 softmax; the probabilities are rounded to fp16 and a value enters P.V
    as fp16(code * v_scale[key]); fp32 accumulation."""
    if _compiling(q_out, k_cache, v_cache, k_scale, v_scale, pos):
        out = _decode_attn_kv8_op(q_out, k_cache, v_cache, k_scale, v_scale, pos, scale, max_len, return_fp16)
    else:
        out = _decode_attention_kv8_impl(q_out, k_cache, v_cache, k_scale, v_scale, pos, scale, max_len, return_fp16)
    return out if return_fp16 else out[:2]


# ---- the block-table (paged) KV cache (include/qqq_amd_paged.h): the four ops above over pools of blocks [num_blocks, kvh, block_size, d]
# that any sequence may own -- a slot per token for the write, a block table per row for the decode attention.

def _paged_check_pools(name, k_pool, v_pool, k_scale=None, v_scale=None):
    # (num_blocks, kvh, block_size, d); an int8 pool comes with its scales
    kv8 = k_scale is not None
    want = torch.int8 if kv8 else torch.float16
    if k_pool.dtype != want or v_pool.dtype != want or (kv8 and any(t.dtype != torch.float32 for t in (k_scale, v_scale))):
        raise RuntimeError(f"{name}: the pools must be {'int8 and their scales f32' if kv8 else 'fp16'}")
    if k_pool.dim() != 4:
        raise RuntimeError(f"{name}: k_pool must be [num_blocks, kvh, block_size, d]")
    if v_pool.shape != k_pool.shape or (kv8 and (k_scale.shape != k_pool.shape[:3] or v_scale.shape != k_pool.shape[:3])):
        raise RuntimeError(f"{name}: v_pool must have k_pool's shape [num_blocks, kvh, block_size, d]" +
                           (" and the scales its first three dimensions" if kv8 else ""))
    for nm, t in (("k_pool", k_pool), ("v_pool", v_pool)) + ((("k_scale", k_scale), ("v_scale", v_scale)) if kv8 else ()):
        if not t.is_contiguous():
            raise RuntimeError(f"{name}: {nm} must be contiguous")
    return tuple(k_pool.shape)


def _rope_qkv_paged_shapes(name, q, k, v, cos, pos, slots, k_pool):
    # (m, h, kvh, d, num_blocks, block_size) from the tensors' shapes; raises for anything the kernel could not take
    if k_pool.dim() != 4:
        raise RuntimeError(f"{name}: k_pool must be [num_blocks, kvh, block_size, d]")
    nb, kvh, bs, d = k_pool.shape
    m = pos.numel()
    if slots.numel() != m:
        raise RuntimeError(f"{name}: pos holds {m} positions and slots {slots.numel()} slots")
    if m == 0 or d == 0:
        return m, 0, kvh, d, nb, bs
    if q.numel() % (m * d) or k.numel() != m * kvh * d or v.numel() != m * kvh * d:
        raise RuntimeError(f"{name}: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} must hold {m} token rows of h*{d}, "
                           f"{kvh}*{d}, {kvh}*{d} elements")
    if cos.dim() != 2 or cos.shape[1] != d:
        raise RuntimeError(f"{name}: cos / sin must be fp16 [table_len, {d}]")
    return m, q.numel() // (m * d), kvh, d, nb, bs


def _rope_qkv_paged_impl(q, k, v, cos, sin, pos, slots, k_pool, v_pool, k_scale=None, v_scale=None):
    kv8 = k_scale is not None
    name = "rope_qkv_paged_kv8" if kv8 else "rope_qkv_paged"
    ts = (q, k, v, cos, sin, pos, slots, k_pool, v_pool) + ((k_scale, v_scale) if kv8 else ())
    _same_gpu(name, ts)
    if any(t.dtype != torch.float16 for t in (q, k, v, cos, sin)) or pos.dtype != torch.int64 or slots.dtype != torch.int64:
        raise RuntimeError(f"{name}: q, k, v, cos and sin must be fp16, pos and slots int64")
    _paged_check_pools(name, k_pool, v_pool, k_scale, v_scale)
    m, h, kvh, d, nb, bs = _rope_qkv_paged_shapes(name, q, k, v, cos, pos, slots, k_pool)
    if sin.shape != cos.shape:
        raise RuntimeError(f"{name}: sin must have cos's shape")
    q_out = torch.empty((m, h, d), dtype=torch.float16, device=q.device)
    if q_out.numel() == 0:
        return q_out
    (q2, ld_q), (k2, ld_k), (v2, ld_v) = _rows(q, h * d), _rows(k, kvh * d), _rows(v, kvh * d)
    cos, sin, pos, slots = cos.contiguous(), sin.contiguous(), pos.contiguous(), slots.contiguous()
    L = _lib.lib()
    head = (_ptr(q2), ld_q, _ptr(k2), ld_k, _ptr(v2), ld_v, _ptr(cos), _ptr(sin), cos.shape[0], _ptr(pos), _ptr(slots), _ptr(q_out),
            _ptr(k_pool), _ptr(v_pool))
    tail = (m, h, kvh, d, nb, bs, q.device.index or 0, _stream_for(q))
    if kv8:
        err = L.qqq_rope_qkv_paged_kv8(*head, _ptr(k_scale), _ptr(v_scale), *tail)
    else:
        err = L.qqq_rope_qkv_paged(*head, *tail)
    _raise_lib(name, err)
    return q_out


@torch.library.custom_op("qqq_amd::rope_qkv_paged", mutates_args=("k_pool", "v_pool"))
def _rope_qkv_paged_op(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor,
                       slots: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor) -> torch.Tensor:
    return _rope_qkv_paged_impl(q, k, v, cos, sin, pos, slots, k_pool, v_pool)


@_rope_qkv_paged_op.register_fake
def _(q, k, v, cos, sin, pos, slots, k_pool, v_pool):
    m, h, _, d, _, _ = _rope_qkv_paged_shapes("rope_qkv_paged", q, k, v, cos, pos, slots, k_pool)
    return q.new_empty((m, h, d), dtype=torch.float16)


def rope_qkv_paged(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor,
                   slots: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor) -> torch.Tensor:
    """rope_qkv into a block pool, one launch for all m tokens of the call (any mix of sequences): q_out and the cached rows are rope_qkv's
    for the same token and position, bit for bit.

    q, k, v, cos, sin   as for rope_qkv (head_dim 64 or 128);  pos  int64 [m], a position per token
    slots      int64 [m]: token t's k / v rows go to block slots[t] // block_size at offset slots[t] % block_size
    k_pool, v_pool   fp16 [num_blocks, kvh, block_size, d] (block_size a power of two in [16, 256]), updated in place
    Returns q_out fp16 [m, h, d], token-major (for a decode batch the memory of [b, h, 1, d]).  A token whose position is outside
    [0, table_len) writes nothing; a token whose slot is outside the pool (a padding slot, -1) writes its q_out row only."""
    ts = (q, k, v, cos, sin, pos, slots, k_pool, v_pool)
    if _compiling(*ts):
        return _rope_qkv_paged_op(*ts)
    return _rope_qkv_paged_impl(*ts)


@torch.library.custom_op("qqq_amd::rope_qkv_paged_kv8", mutates_args=("k_pool", "v_pool", "k_scale", "v_scale"))
def _rope_qkv_paged_kv8_op(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor,
                           slots: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale: torch.Tensor,
                           v_scale: torch.Tensor) -> torch.Tensor:
    return _rope_qkv_paged_impl(q, k, v, cos, sin, pos, slots, k_pool, v_pool, k_scale, v_scale)


@_rope_qkv_paged_kv8_op.register_fake
def _(q, k, v, cos, sin, pos, slots, k_pool, v_pool, k_scale, v_scale):
    m, h, _, d, _, _ = _rope_qkv_paged_shapes("rope_qkv_paged_kv8", q, k, v, cos, pos, slots, k_pool)
    return q.new_empty((m, h, d), dtype=torch.float16)


def rope_qkv_paged_kv8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor,
                       slots: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale: torch.Tensor,
                       v_scale: torch.Tensor) -> torch.Tensor:
    """rope_qkv_paged into an int8 pool: every cached row is stored as rope_qkv_kv8 stores it (codes and one f32 scale), bit for bit.

    k_pool, v_pool  int8 [num_blocks, kvh, block_size, d];  k_scale, v_scale  f32 [num_blocks, kvh, block_size]; all four updated in place
    Everything else, the return value and the padding / out-of-range rules are rope_qkv_paged's."""
    ts = (q, k, v, cos, sin, pos, slots, k_pool, v_pool, k_scale, v_scale)
    if _compiling(*ts):
        return _rope_qkv_paged_kv8_op(*ts)
    return _rope_qkv_paged_impl(*ts)


# ---- Qwen3's per-head q / k RMSNorm fused into the four RoPE / cache-write ops above (include_ops/qqq_amd_qknorm.h): still one launch each.

def _qknorm_check(name, q, k, v, cos, sin, idx, q_weight, k_weight, eps, d):
    if any(t.dtype != torch.float16 for t in (q, k, v, cos, sin, q_weight, k_weight)) or any(t.dtype != torch.int64 for t in idx):
        raise RuntimeError(f"{name}: q, k, v, cos, sin and the norm weights must be fp16, {' and '.join(('pos', 'slots')[:len(idx)])} int64")
    if d not in (64, 128):
        raise RuntimeError(f"{name}: head_dim {d} is not supported (the fused q / k norm takes 64 or 128)")
    if q_weight.shape != (d,) or k_weight.shape != (d,):
        raise RuntimeError(f"{name}: q_weight {tuple(q_weight.shape)} and k_weight {tuple(k_weight.shape)} must be fp16 [{d}]")
    if sin.shape != cos.shape:
        raise RuntimeError(f"{name}: sin must have cos's shape")
    if not (0.0 <= float(eps) < float("inf")):
        raise RuntimeError(f"{name}: eps {eps} must be finite and >= 0")


def _norm_weight(w):
    # [d] fp16 where the kernel can read it: contiguous, 16-byte aligned (a copy otherwise; a Parameter's storage is both)
    w = w.contiguous()
    return w if w.data_ptr() % 16 == 0 else w.clone()


def _rope_qkv_norm_impl(q, k, v, q_weight, k_weight, eps, cos, sin, pos, k_cache, v_cache, k_scale=None, v_scale=None):
    kv8 = k_scale is not None
    name = "rope_qkv_norm_kv8" if kv8 else "rope_qkv_norm"
    ts = (q, k, v, q_weight, k_weight, cos, sin, pos, k_cache, v_cache) + ((k_scale, v_scale) if kv8 else ())
    _same_gpu(name, ts)
    if kv8:
        _kv8_check_caches(name, k_cache, v_cache, k_scale, v_scale)
    else:
        if k_cache.dtype != torch.float16 or v_cache.dtype != torch.float16 or k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
            raise RuntimeError(f"{name}: k_cache and v_cache must be fp16 [b, kvh, cap, d] of one shape")
        for nm, t in (("k_cache", k_cache), ("v_cache", v_cache)):
            if not t.is_contiguous():
                raise RuntimeError(f"{name}: {nm} must be contiguous (it is written in place)")
    try:
        b, s, h, kvh, d, cap = _rope_qkv_shapes(q, k, v, cos, pos, k_cache)
    except RuntimeError as e:
        raise RuntimeError(str(e).replace("rope_qkv:", name + ":", 1)) from None
    _qknorm_check(name, q, k, v, cos, sin, (pos,), q_weight, k_weight, eps, d)
    q_out = torch.empty((b, h, s, d), dtype=torch.float16, device=q.device)
    if q_out.numel() == 0:
        return q_out
    (q2, ld_q), (k2, ld_k), (v2, ld_v) = _rows(q, h * d), _rows(k, kvh * d), _rows(v, kvh * d)
    cos, sin, pos, qw, kw = cos.contiguous(), sin.contiguous(), pos.contiguous(), _norm_weight(q_weight), _norm_weight(k_weight)
    L = _lib.lib()
    head = (_ptr(q2), ld_q, _ptr(k2), ld_k, _ptr(v2), ld_v, _ptr(qw), _ptr(kw), float(eps), _ptr(cos), _ptr(sin), cos.shape[0], _ptr(pos),
            _ptr(q_out), _ptr(k_cache), _ptr(v_cache))
    tail = (b, s, h, kvh, d, cap, q.device.index or 0, _stream_for(q))
    if kv8:
        err = L.qqq_rope_qkv_norm_kv8(*head, _ptr(k_scale), _ptr(v_scale), *tail)
    else:
        err = L.qqq_rope_qkv_norm(*head, *tail)
    _raise_lib(name, err)
    return q_out


@torch.library.custom_op("qqq_amd::rope_qkv_norm", mutates_args=("k_cache", "v_cache"))
def _rope_qkv_norm_op(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_weight: torch.Tensor, k_weight: torch.Tensor, eps: float,
                      cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor,
                      v_cache: torch.Tensor) -> torch.Tensor:
    return _rope_qkv_norm_impl(q, k, v, q_weight, k_weight, eps, cos, sin, pos, k_cache, v_cache)


@_rope_qkv_norm_op.register_fake
def _(q, k, v, q_weight, k_weight, eps, cos, sin, pos, k_cache, v_cache):
    b, s, h, _, d, _ = _rope_qkv_shapes(q, k, v, cos, pos, k_cache)
    return q.new_empty((b, h, s, d), dtype=torch.float16)


def rope_qkv_norm(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_weight: torch.Tensor, k_weight: torch.Tensor, eps: float,
                  cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor) -> torch.Tensor:
    """rope_qkv with Qwen3's per-head RMSNorm of q and k in front of the rotation, one launch: every q / k head row x becomes
    fp16(w * fp16(x * rsqrt(mean(x^2) + eps))) -- transformers' Qwen3RMSNorm on fp16, the mean in f64 in the order
    include_ops/qqq_amd_qknorm.h states -- and is then rotated and stored exactly as rope_qkv does; v is untouched.

    q_weight, k_weight   fp16 [head_dim]: q_norm.weight and k_norm.weight;  eps  rms_norm_eps;  head_dim 64 or 128
    Everything else, the return value and the out-of-range rule are rope_qkv's."""
    ts = (q, k, v, q_weight, k_weight, cos, sin, pos, k_cache, v_cache)
    if _compiling(*ts):
        return _rope_qkv_norm_op(q, k, v, q_weight, k_weight, float(eps), cos, sin, pos, k_cache, v_cache)
    return _rope_qkv_norm_impl(q, k, v, q_weight, k_weight, eps, cos, sin, pos, k_cache, v_cache)


@torch.library.custom_op("qqq_amd::rope_qkv_norm_kv8", mutates_args=("k_cache", "v_cache", "k_scale", "v_scale"))
def _rope_qkv_norm_kv8_op(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_weight: torch.Tensor, k_weight: torch.Tensor, eps: float,
                          cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                          k_scale: torch.Tensor, v_scale: torch.Tensor) -> torch.Tensor:
    return _rope_qkv_norm_impl(q, k, v, q_weight, k_weight, eps, cos, sin, pos, k_cache, v_cache, k_scale, v_scale)


@_rope_qkv_norm_kv8_op.register_fake
def _(q, k, v, q_weight, k_weight, eps, cos, sin, pos, k_cache, v_cache, k_scale, v_scale):
    b, s, h, _, d, _ = _rope_qkv_shapes(q, k, v, cos, pos, k_cache)
    return q.new_empty((b, h, s, d), dtype=torch.float16)


def rope_qkv_norm_kv8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_weight: torch.Tensor, k_weight: torch.Tensor, eps: float,
                      cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                      k_scale: torch.Tensor, v_scale: torch.Tensor) -> torch.Tensor:
    """rope_qkv_norm into an int8 cache: q_out is rope_qkv_norm's, every cached row is dynamic_quant of the fp16 row rope_qkv_norm would
    have cached, bit for bit.  The caches and scales are rope_qkv_kv8's."""
    ts = (q, k, v, q_weight, k_weight, cos, sin, pos, k_cache, v_cache, k_scale, v_scale)
    if _compiling(*ts):
        return _rope_qkv_norm_kv8_op(q, k, v, q_weight, k_weight, float(eps), cos, sin, pos, k_cache, v_cache, k_scale, v_scale)
    return _rope_qkv_norm_impl(q, k, v, q_weight, k_weight, eps, cos, sin, pos, k_cache, v_cache, k_scale, v_scale)


def _rope_qkv_norm_paged_impl(q, k, v, q_weight, k_weight, eps, cos, sin, pos, slots, k_pool, v_pool, k_scale=None, v_scale=None):
    kv8 = k_scale is not None
    name = "rope_qkv_norm_paged_kv8" if kv8 else "rope_qkv_norm_paged"
    ts = (q, k, v, q_weight, k_weight, cos, sin, pos, slots, k_pool, v_pool) + ((k_scale, v_scale) if kv8 else ())
    _same_gpu(name, ts)
    _paged_check_pools(name, k_pool, v_pool, k_scale, v_scale)
    m, h, kvh, d, nb, bs = _rope_qkv_paged_shapes(name, q, k, v, cos, pos, slots, k_pool)
    _qknorm_check(name, q, k, v, cos, sin, (pos, slots), q_weight, k_weight, eps, d)
    q_out = torch.empty((m, h, d), dtype=torch.float16, device=q.device)
    if q_out.numel() == 0:
        return q_out
    (q2, ld_q), (k2, ld_k), (v2, ld_v) = _rows(q, h * d), _rows(k, kvh * d), _rows(v, kvh * d)
    cos, sin, pos, slots = cos.contiguous(), sin.contiguous(), pos.contiguous(), slots.contiguous()
    qw, kw = _norm_weight(q_weight), _norm_weight(k_weight)
    L = _lib.lib()
    head = (_ptr(q2), ld_q, _ptr(k2), ld_k, _ptr(v2), ld_v, _ptr(qw), _ptr(kw), float(eps), _ptr(cos), _ptr(sin), cos.shape[0], _ptr(pos),
            _ptr(slots), _ptr(q_out), _ptr(k_pool), _ptr(v_pool))
    tail = (m, h, kvh, d, nb, bs, q.device.index or 0, _stream_for(q))
    if kv8:
        err = L.qqq_rope_qkv_norm_paged_kv8(*head, _ptr(k_scale), _ptr(v_scale), *tail)
    else:
        err = L.qqq_rope_qkv_norm_paged(*head, *tail)
    _raise_lib(name, err)
    return q_out


@torch.library.custom_op("qqq_amd::rope_qkv_norm_paged", mutates_args=("k_pool", "v_pool"))
def _rope_qkv_norm_paged_op(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_weight: torch.Tensor, k_weight: torch.Tensor, eps: float,
                            cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor, k_pool: torch.Tensor,
                            v_pool: torch.Tensor) -> torch.Tensor:
    return _rope_qkv_norm_paged_impl(q, k, v, q_weight, k_weight, eps, cos, sin, pos, slots, k_pool, v_pool)


@_rope_qkv_norm_paged_op.register_fake
def _(q, k, v, q_weight, k_weight, eps, cos, sin, pos, slots, k_pool, v_pool):
    m, h, _, d, _, _ = _rope_qkv_paged_shapes("rope_qkv_norm_paged", q, k, v, cos, pos, slots, k_pool)
    return q.new_empty((m, h, d), dtype=torch.float16)


def rope_qkv_norm_paged(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_weight: torch.Tensor, k_weight: torch.Tensor, eps: float,
                        cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor, k_pool: torch.Tensor,
                        v_pool: torch.Tensor) -> torch.Tensor:
    """rope_qkv_paged with Qwen3's per-head RMSNorm of q and k in front of the rotation (rope_qkv_norm's arithmetic), one launch for all m
    tokens.  q_weight, k_weight fp16 [head_dim], eps rms_norm_eps; everything else, the return value and the padding / out-of-range
    rules are rope_qkv_paged's."""
    ts = (q, k, v, q_weight, k_weight, cos, sin, pos, slots, k_pool, v_pool)
    if _compiling(*ts):
        return _rope_qkv_norm_paged_op(q, k, v, q_weight, k_weight, float(eps), cos, sin, pos, slots, k_pool, v_pool)
    return _rope_qkv_norm_paged_impl(q, k, v, q_weight, k_weight, eps, cos, sin, pos, slots, k_pool, v_pool)


@torch.library.custom_op("qqq_amd::rope_qkv_norm_paged_kv8", mutates_args=("k_pool", "v_pool", "k_scale", "v_scale"))
def _rope_qkv_norm_paged_kv8_op(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_weight: torch.Tensor, k_weight: torch.Tensor,
                                eps: float, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor,
                                k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor) -> torch.Tensor:
    return _rope_qkv_norm_paged_impl(q, k, v, q_weight, k_weight, eps, cos, sin, pos, slots, k_pool, v_pool, k_scale, v_scale)


@_rope_qkv_norm_paged_kv8_op.register_fake
def _(q, k, v, q_weight, k_weight, eps, cos, sin, pos, slots, k_pool, v_pool, k_scale, v_scale):
    m, h, _, d, _, _ = _rope_qkv_paged_shapes("rope_qkv_norm_paged_kv8", q, k, v, cos, pos, slots, k_pool)
    return q.new_empty((m, h, d), dtype=torch.float16)


def rope_qkv_norm_paged_kv8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_weight: torch.Tensor, k_weight: torch.Tensor, eps: float,
                            cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor, k_pool: torch.Tensor,
                            v_pool: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor) -> torch.Tensor:
    """rope_qkv_norm_paged into an int8 pool: every cached row as rope_qkv_norm_kv8 stores it, bit for bit.  The pools and scales are
    rope_qkv_paged_kv8's."""
    ts = (q, k, v, q_weight, k_weight, cos, sin, pos, slots, k_pool, v_pool, k_scale, v_scale)
    if _compiling(*ts):
        return _rope_qkv_norm_paged_kv8_op(q, k, v, q_weight, k_weight, float(eps), cos, sin, pos, slots, k_pool, v_pool, k_scale, v_scale)
    return _rope_qkv_norm_paged_impl(q, k, v, q_weight, k_weight, eps, cos, sin, pos, slots, k_pool, v_pool, k_scale, v_scale)


def _decode_attention_paged_shapes(name, q_out, k_pool, block_table, pos, max_len):
    # (b, h, kvh, d, num_blocks, block_size, table_stride, max_len) from the tensors' shapes
    if k_pool.dim() != 4:
        raise RuntimeError(f"{name}: k_pool must be [num_blocks, kvh, block_size, d]")
    nb, kvh, bs, d = k_pool.shape
    if block_table.dim() != 2:
        raise RuntimeError(f"{name}: block_table must be int32 [b, blocks per row]")
    b, width = block_table.shape
    if q_out.dim() == 4 and q_out.shape[2] == 1:
        q_out = q_out[:, :, 0]
    if q_out.dim() != 3 or q_out.shape[0] != b or q_out.shape[2] != d:
        raise RuntimeError(f"{name}: q_out {tuple(q_out.shape)} must be [{b}, h, {d}] or [{b}, h, 1, {d}] (rope_qkv_paged's output of a "
                           f"decode batch)")
    if pos.numel() != b:
        raise RuntimeError(f"{name}: pos holds {pos.numel()} positions, the block table has {b} rows")
    max_len = width * bs if max_len is None else int(max_len)
    return b, q_out.shape[1], kvh, d, nb, bs, width, max_len


def _decode_attention_paged_impl(q_out, k_pool, v_pool, block_table, pos, scale, max_len, return_fp16, k_scale=None, v_scale=None):
    kv8 = k_scale is not None
    name = "decode_attention_paged_kv8" if kv8 else "decode_attention_paged"
    ts = (q_out, k_pool, v_pool, block_table, pos) + ((k_scale, v_scale) if kv8 else ())
    _same_gpu(name, ts)
    if q_out.dtype != torch.float16 or pos.dtype != torch.int64 or block_table.dtype != torch.int32:
        raise RuntimeError(f"{name}: q_out must be fp16, pos int64 and block_table int32")
    _paged_check_pools(name, k_pool, v_pool, k_scale, v_scale)
    b, h, kvh, d, nb, bs, width, max_len = _decode_attention_paged_shapes(name, q_out, k_pool, block_table, pos, max_len)
    dev = q_out.device
    xq = torch.empty((b, h * d), dtype=torch.int8, device=dev)
    s1 = torch.empty((b, 1), dtype=torch.float32, device=dev)
    o16 = torch.empty((b, h * d) if return_fp16 else (0,), dtype=torch.float16, device=dev)
    if b == 0:
        return xq, s1, o16
    L = _lib.lib()
    nbytes = L.qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len)
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)  # torch's allocator: also under stream / graph capture
    q2, pos, table = q_out.contiguous(), pos.contiguous(), block_table.contiguous()
    tail = (_ptr(table), width, _ptr(pos), float(scale), _ptr(o16), _ptr(xq), _ptr(s1), _ptr(ws), ws.numel(), b, h, kvh, d, nb, bs, max_len,
            dev.index or 0, _stream_for(q_out))
    if kv8:
        err = L.qqq_decode_attn_paged_kv8(_ptr(q2), _ptr(k_pool), _ptr(v_pool), _ptr(k_scale), _ptr(v_scale), *tail)
    else:
        err = L.qqq_decode_attn_paged(_ptr(q2), _ptr(k_pool), _ptr(v_pool), *tail)
    _raise_lib(name, err)
    return xq, s1, o16


def _decode_paged_fake(name, q_out, k_pool, block_table, pos, max_len, return_fp16):
    b, h, _, d = _decode_attention_paged_shapes(name, q_out, k_pool, block_table, pos, max_len)[:4]
    return (q_out.new_empty((b, h * d), dtype=torch.int8), q_out.new_empty((b, 1), dtype=torch.float32),
            q_out.new_empty((b, h * d) if return_fp16 else (0,), dtype=torch.float16))


@torch.library.custom_op("qqq_amd::decode_attn_paged", mutates_args=())
def _decode_attn_paged_op(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor, pos: torch.Tensor,
                          scale: float, max_len: Optional[int], return_fp16: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _decode_attention_paged_impl(q_out, k_pool, v_pool, block_table, pos, scale, max_len, return_fp16)


@_decode_attn_paged_op.register_fake
def _(q_out, k_pool, v_pool, block_table, pos, scale, max_len, return_fp16):
    return _decode_paged_fake("decode_attention_paged", q_out, k_pool, block_table, pos, max_len, return_fp16)


def decode_attention_paged(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor, pos: torch.Tensor,
                           scale: float, max_len: Optional[int] = None, return_fp16: bool = False):
    """decode_attention over a block pool: (xq int8 [b, h*d], s1 f32 [b, 1]), plus the fp16 output [b, h*d] with `return_fp16` -- bit for bit
    decode_attention's over a contiguous cache that holds the same rows, for equal b and max_len.

    q_out      fp16 [b, h, d] or [b, h, 1, d]: rope_qkv_paged's output of a decode batch
    k_pool, v_pool   fp16 [num_blocks, kvh, block_size, d], only read
    block_table      int32 [b, W] in device memory: key j of row bi lives in block block_table[bi, j // block_size]; only the entries up to
                     pos[bi] // block_size are read, several rows may name the same blocks, ids are clamped into the pool
    pos        int64 [b]: row bi attends keys 0 ... pos[bi];  scale  the score scale
    max_len    the launch is sized for positions below it (default and upper bound: W * block_size); a row whose position is outside
               [0, max_len) writes nothing"""
    if _compiling(q_out, k_pool, v_pool, block_table, pos):
        out = _decode_attn_paged_op(q_out, k_pool, v_pool, block_table, pos, scale, max_len, return_fp16)
    else:
        out = _decode_attention_paged_impl(q_out, k_pool, v_pool, block_table, pos, scale, max_len, return_fp16)
    return out if return_fp16 else out[:2]


@torch.library.custom_op("qqq_amd::decode_attn_paged_kv8", mutates_args=())
def _decode_attn_paged_kv8_op(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                              block_table: torch.Tensor, pos: torch.Tensor, scale: float, max_len: Optional[int],
                              return_fp16: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _decode_attention_paged_impl(q_out, k_pool, v_pool, block_table, pos, scale, max_len, return_fp16, k_scale, v_scale)


@_decode_attn_paged_kv8_op.register_fake
def _(q_out, k_pool, v_pool, k_scale, v_scale, block_table, pos, scale, max_len, return_fp16):
    return _decode_paged_fake("decode_attention_paged_kv8", q_out, k_pool, block_table, pos, max_len, return_fp16)


def decode_attention_paged_kv8(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                               block_table: torch.Tensor, pos: torch.Tensor, scale: float, max_len: Optional[int] = None,
                               return_fp16: bool = False):
    """decode_attention_paged over an int8 pool (k_pool, v_pool int8 [num_blocks, kvh, block_size, d]; k_scale, v_scale f32 [num_blocks, kvh,
    block_size]) with decode_attention_kv8's arithmetic, bit for bit."""
    if _compiling(q_out, k_pool, v_pool, k_scale, v_scale, block_table, pos):
        out = _decode_attn_paged_kv8_op(q_out, k_pool, v_pool, k_scale, v_scale, block_table, pos, scale, max_len, return_fp16)
    else:
        out = _decode_attention_paged_impl(q_out, k_pool, v_pool, block_table, pos, scale, max_len, return_fp16, k_scale, v_scale)
    return out if return_fp16 else out[:2]


# ---- the decode attention of sibling rows over a shared prefix (include/qqq_amd_shared.h): the n completions of one prompt read the
# prompt's keys once per pack of rows; every row bit for bit decode_attention_paged(_kv8)'s.

def _decode_attention_paged_shared_check(name, block_table, family, shared, pack):
    b = block_table.shape[0] if block_table.dim() == 2 else -1
    if family.dtype != torch.int32 or shared.dtype != torch.int64:
        raise RuntimeError(f"{name}: family must be int32 and shared int64")
    if family.numel() != b or shared.numel() != b:
        raise RuntimeError(f"{name}: family holds {family.numel()} and shared {shared.numel()} entries, the block table has {b} rows")
    if int(pack) < 1:
        raise RuntimeError(f"{name}: pack must be at least 1, not {pack}")


def _decode_attention_paged_shared_impl(q_out, k_pool, v_pool, block_table, pos, family, shared, pack, scale, max_len, return_fp16,
                                        k_scale=None, v_scale=None):
    kv8 = k_scale is not None
    name = "decode_attention_paged_shared_kv8" if kv8 else "decode_attention_paged_shared"
    ts = (q_out, k_pool, v_pool, block_table, pos, family, shared) + ((k_scale, v_scale) if kv8 else ())
    _same_gpu(name, ts)
    if q_out.dtype != torch.float16 or pos.dtype != torch.int64 or block_table.dtype != torch.int32:
        raise RuntimeError(f"{name}: q_out must be fp16, pos int64 and block_table int32")
    _paged_check_pools(name, k_pool, v_pool, k_scale, v_scale)
    b, h, kvh, d, nb, bs, width, max_len = _decode_attention_paged_shapes(name, q_out, k_pool, block_table, pos, max_len)
    _decode_attention_paged_shared_check(name, block_table, family, shared, pack)
    dev = q_out.device
    xq = torch.empty((b, h * d), dtype=torch.int8, device=dev)
    s1 = torch.empty((b, 1), dtype=torch.float32, device=dev)
    o16 = torch.empty((b, h * d) if return_fp16 else (0,), dtype=torch.float16, device=dev)
    if b == 0:
        return xq, s1, o16
    L = _lib.lib()
    nbytes = L.qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len)
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)  # torch's allocator: also under stream / graph capture
    q2, pos, table = q_out.contiguous(), pos.contiguous(), block_table.contiguous()
    family, shared = family.contiguous(), shared.contiguous()
    tail = (_ptr(table), width, _ptr(pos), _ptr(family), _ptr(shared), int(pack), float(scale), _ptr(o16), _ptr(xq), _ptr(s1), _ptr(ws),
            ws.numel(), b, h, kvh, d, nb, bs, max_len, dev.index or 0, _stream_for(q_out))
    if kv8:
        err = L.qqq_decode_attn_paged_shared_kv8(_ptr(q2), _ptr(k_pool), _ptr(v_pool), _ptr(k_scale), _ptr(v_scale), *tail)
    else:
        err = L.qqq_decode_attn_paged_shared(_ptr(q2), _ptr(k_pool), _ptr(v_pool), *tail)
    _raise_lib(name, err)
    return xq, s1, o16


def _decode_paged_shared_fake(name, q_out, k_pool, block_table, pos, family, shared, pack, max_len, return_fp16):
    _decode_attention_paged_shared_check(name, block_table, family, shared, pack)
    return _decode_paged_fake(name, q_out, k_pool, block_table, pos, max_len, return_fp16)


@torch.library.custom_op("qqq_amd::decode_attn_paged_shared", mutates_args=())
def _decode_attn_paged_shared_op(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor,
                                 pos: torch.Tensor, family: torch.Tensor, shared: torch.Tensor, pack: int, scale: float,
                                 max_len: Optional[int], return_fp16: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _decode_attention_paged_shared_impl(q_out, k_pool, v_pool, block_table, pos, family, shared, pack, scale, max_len, return_fp16)


@_decode_attn_paged_shared_op.register_fake
def _(q_out, k_pool, v_pool, block_table, pos, family, shared, pack, scale, max_len, return_fp16):
    return _decode_paged_shared_fake("decode_attention_paged_shared", q_out, k_pool, block_table, pos, family, shared, pack, max_len,
                                     return_fp16)


def decode_attention_paged_shared(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor,
                                  pos: torch.Tensor, family: torch.Tensor, shared: torch.Tensor, pack: int, scale: float,
                                  max_len: Optional[int] = None, return_fp16: bool = False):
    """decode_attention_paged for rows that share a prefix of their block tables (PagedKVCache.fork): every row's xq, s1 and fp16 output bit
    for bit decode_attention_paged's on the same tensors, the splits inside a family's shared keys read once per pack of rows.

    q_out, k_pool, v_pool, block_table, pos, scale, max_len   as for decode_attention_paged
    family     int32 [b]: the index of the first row of row i's family (siblings are adjacent; a lone row names itself)
    shared     int64 [b]: the leading keys a row has in common with its family, the same on all its rows (0 for a lone row); the rows of a
               family hold equal table entries for their first shared // block_size blocks
    pack       sibling rows whose queries share one workgroup: pack >= 1, (h // kvh) * pack <= 64; pack = 1 is decode_attention_paged
    A row whose position is outside [0, max_len) writes nothing and does not disturb its siblings; descriptors that make no sense make
    rows compute alone."""
    ts = (q_out, k_pool, v_pool, block_table, pos, family, shared)
    if _compiling(*ts):
        out = _decode_attn_paged_shared_op(*ts, pack, scale, max_len, return_fp16)
    else:
        out = _decode_attention_paged_shared_impl(*ts, pack, scale, max_len, return_fp16)
    return out if return_fp16 else out[:2]


@torch.library.custom_op("qqq_amd::decode_attn_paged_shared_kv8", mutates_args=())
def _decode_attn_paged_shared_kv8_op(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale: torch.Tensor,
                                     v_scale: torch.Tensor, block_table: torch.Tensor, pos: torch.Tensor, family: torch.Tensor,
                                     shared: torch.Tensor, pack: int, scale: float, max_len: Optional[int],
                                     return_fp16: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _decode_attention_paged_shared_impl(q_out, k_pool, v_pool, block_table, pos, family, shared, pack, scale, max_len, return_fp16,
                                               k_scale, v_scale)


@_decode_attn_paged_shared_kv8_op.register_fake
def _(q_out, k_pool, v_pool, k_scale, v_scale, block_table, pos, family, shared, pack, scale, max_len, return_fp16):
    return _decode_paged_shared_fake("decode_attention_paged_shared_kv8", q_out, k_pool, block_table, pos, family, shared, pack, max_len,
                                     return_fp16)


def decode_attention_paged_shared_kv8(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale: torch.Tensor,
                                      v_scale: torch.Tensor, block_table: torch.Tensor, pos: torch.Tensor, family: torch.Tensor,
                                      shared: torch.Tensor, pack: int, scale: float, max_len: Optional[int] = None,
                                      return_fp16: bool = False):
    """decode_attention_paged_shared over an int8 pool: every row bit for bit decode_attention_paged_kv8's."""
    if _compiling(q_out, k_pool, v_pool, k_scale, v_scale, block_table, pos, family, shared):
        out = _decode_attn_paged_shared_kv8_op(q_out, k_pool, v_pool, k_scale, v_scale, block_table, pos, family, shared, pack, scale,
                                               max_len, return_fp16)
    else:
        out = _decode_attention_paged_shared_impl(q_out, k_pool, v_pool, block_table, pos, family, shared, pack, scale, max_len,
                                                  return_fp16, k_scale, v_scale)
    return out if return_fp16 else out[:2]


def decode_attention_shared_plan(b: int, h: int, kvh: int, max_len: int, pack: int):
    """(splits, chunk) of a decode_attention_paged_shared call on the current device: split s covers keys s * chunk ... (s + 1) * chunk - 1
    and is taken jointly by siblings that share at least (s + 1) * chunk keys."""
    import ctypes

    L = _lib.lib()
    splits, chunk = ctypes.c_int(0), ctypes.c_int(0)
    _raise_lib("decode_attention_shared_plan", L.qqq_decode_attn_shared_plan(int(b), int(h), int(kvh), int(max_len), int(pack),
                                                                             ctypes.byref(splits), ctypes.byref(chunk)))
    return splits.value, chunk.value


# ---- the paged prefill attention (include/qqq_amd_prefill.h): any mix of prompts, chunks and decoding rows of a packed batch in one call,
# K and V read in place through the block table.

def _prefill_attention_paged_shapes(name, q_out, k_pool, block_table, cu_tokens, start_pos, max_len):
    # (m, b, h, kvh, d, num_blocks, block_size, table_stride, max_len) from the tensors' shapes
    if k_pool.dim() != 4:
        raise RuntimeError(f"{name}: k_pool must be [num_blocks, kvh, block_size, d]")
    nb, kvh, bs, d = k_pool.shape
    if block_table.dim() != 2:
        raise RuntimeError(f"{name}: block_table must be int32 [b, blocks per row]")
    b, width = block_table.shape
    if q_out.dim() != 3 or q_out.shape[2] != d:
        raise RuntimeError(f"{name}: q_out {tuple(q_out.shape)} must be [m, h, {d}] (rope_qkv_paged's output)")
    if cu_tokens.numel() != b + 1 or start_pos.numel() != b:
        raise RuntimeError(f"{name}: cu_tokens holds {cu_tokens.numel()} entries and start_pos {start_pos.numel()}, the block table has {b} "
                           f"rows (need b + 1 and b)")
    max_len = width * bs if max_len is None else int(max_len)
    return q_out.shape[0], b, q_out.shape[1], kvh, d, nb, bs, width, max_len


def _prefill_attention_paged_impl(q_out, k_pool, v_pool, block_table, cu_tokens, start_pos, scale, max_len, return_fp16, k_scale=None,
                                  v_scale=None):
    kv8 = k_scale is not None
    name = "prefill_attention_paged_kv8" if kv8 else "prefill_attention_paged"
    ts = (q_out, k_pool, v_pool, block_table, cu_tokens, start_pos) + ((k_scale, v_scale) if kv8 else ())
    _same_gpu(name, ts)
    if q_out.dtype != torch.float16 or start_pos.dtype != torch.int64 or block_table.dtype != torch.int32 or cu_tokens.dtype != torch.int32:
        raise RuntimeError(f"{name}: q_out must be fp16, start_pos int64, block_table and cu_tokens int32")
    _paged_check_pools(name, k_pool, v_pool, k_scale, v_scale)
    m, b, h, kvh, d, nb, bs, width, max_len = _prefill_attention_paged_shapes(name, q_out, k_pool, block_table, cu_tokens, start_pos, max_len)
    dev = q_out.device
    xq = torch.empty((m, h * d), dtype=torch.int8, device=dev)
    s1 = torch.empty((m, 1), dtype=torch.float32, device=dev)
    o16 = torch.empty((m, h * d) if return_fp16 else (0,), dtype=torch.float16, device=dev)
    if m == 0 or b == 0:
        return xq, s1, o16
    L = _lib.lib()
    nbytes = 0 if return_fp16 else L.qqq_prefill_attn_workspace_bytes(m, h, d)
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)  # torch's allocator: also under stream / graph capture
    q2, table, cu, sp = q_out.contiguous(), block_table.contiguous(), cu_tokens.contiguous(), start_pos.contiguous()
    tail = (_ptr(table), width, _ptr(cu), _ptr(sp), float(scale), _ptr(o16), _ptr(xq), _ptr(s1), _ptr(ws), ws.numel(), m, b, h, kvh, d, nb,
            bs, max_len, dev.index or 0, _stream_for(q_out))
    if kv8:
        err = L.qqq_prefill_attn_paged_kv8(_ptr(q2), _ptr(k_pool), _ptr(v_pool), _ptr(k_scale), _ptr(v_scale), *tail)
    else:
        err = L.qqq_prefill_attn_paged(_ptr(q2), _ptr(k_pool), _ptr(v_pool), *tail)
    _raise_lib(name, err)
    return xq, s1, o16


def _prefill_paged_fake(name, q_out, k_pool, block_table, cu_tokens, start_pos, max_len, return_fp16):
    m, _, h, _, d = _prefill_attention_paged_shapes(name, q_out, k_pool, block_table, cu_tokens, start_pos, max_len)[:5]
    return (q_out.new_empty((m, h * d), dtype=torch.int8), q_out.new_empty((m, 1), dtype=torch.float32),
            q_out.new_empty((m, h * d) if return_fp16 else (0,), dtype=torch.float16))


@torch.library.custom_op("qqq_amd::prefill_attn_paged", mutates_args=())
def _prefill_attn_paged_op(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor,
                           cu_tokens: torch.Tensor, start_pos: torch.Tensor, scale: float, max_len: Optional[int],
                           return_fp16: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _prefill_attention_paged_impl(q_out, k_pool, v_pool, block_table, cu_tokens, start_pos, scale, max_len, return_fp16)


@_prefill_attn_paged_op.register_fake
def _(q_out, k_pool, v_pool, block_table, cu_tokens, start_pos, scale, max_len, return_fp16):
    return _prefill_paged_fake("prefill_attention_paged", q_out, k_pool, block_table, cu_tokens, start_pos, max_len, return_fp16)


def prefill_attention_paged(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor,
                            cu_tokens: torch.Tensor, start_pos: torch.Tensor, scale: float, max_len: Optional[int] = None,
                            return_fp16: bool = False):
    """Causal attention of a packed batch of chunks over a block pool, read in place: (xq int8 [m, h*d], s1 f32 [m, 1]) -- o_proj's input,
    bit for bit dynamic_quant of the fp16 output -- plus that output fp16 [m, h*d] with `return_fp16`.  Two launches for the whole batch.

    q_out      fp16 [m, h, d]: rope_qkv_paged's output (the step's new tokens are in the pool already)
    k_pool, v_pool   fp16 [num_blocks, kvh, block_size, d], only read
    block_table      int32 [b, W] in device memory, as for decode_attention_paged
    cu_tokens  int32 [b + 1]: sequence i owns tokens cu_tokens[i] ... cu_tokens[i + 1] - 1 (cu_tokens[0] = 0, non-decreasing); tokens from
               cu_tokens[b] on are padding
    start_pos  int64 [b]: the position of sequence i's first token of the call; token t of it attends keys 0 ... its own position
    max_len    default and upper bound W * block_size; a sequence that starts below 0 or ends beyond max_len writes nothing
    Rows of padding tokens and of such sequences are left as torch.empty made them.  The launch sizes depend on the shapes alone, so a
    captured graph replays with other contents of cu_tokens, start_pos and block_table."""
    if _compiling(q_out, k_pool, v_pool, block_table, cu_tokens, start_pos):
        out = _prefill_attn_paged_op(q_out, k_pool, v_pool, block_table, cu_tokens, start_pos, scale, max_len, return_fp16)
    else:
        out = _prefill_attention_paged_impl(q_out, k_pool, v_pool, block_table, cu_tokens, start_pos, scale, max_len, return_fp16)
    return out if return_fp16 else out[:2]


@torch.library.custom_op("qqq_amd::prefill_attn_paged_kv8", mutates_args=())
def _prefill_attn_paged_kv8_op(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                               block_table: torch.Tensor, cu_tokens: torch.Tensor, start_pos: torch.Tensor, scale: float,
                               max_len: Optional[int], return_fp16: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _prefill_attention_paged_impl(q_out, k_pool, v_pool, block_table, cu_tokens, start_pos, scale, max_len, return_fp16, k_scale,
                                         v_scale)


@_prefill_attn_paged_kv8_op.register_fake
def _(q_out, k_pool, v_pool, k_scale, v_scale, block_table, cu_tokens, start_pos, scale, max_len, return_fp16):
    return _prefill_paged_fake("prefill_attention_paged_kv8", q_out, k_pool, block_table, cu_tokens, start_pos, max_len, return_fp16)


def prefill_attention_paged_kv8(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                                block_table: torch.Tensor, cu_tokens: torch.Tensor, start_pos: torch.Tensor, scale: float,
                                max_len: Optional[int] = None, return_fp16: bool = False):
    """prefill_attention_paged over an int8 pool (k_pool, v_pool int8 [num_blocks, kvh, block_size, d]; k_scale, v_scale f32 [num_blocks,
    kvh, block_size]) with decode_attention_kv8's arithmetic: scores from the codes times the key's scale, V as fp16(code * scale)."""
    if _compiling(q_out, k_pool, v_pool, k_scale, v_scale, block_table, cu_tokens, start_pos):
        out = _prefill_attn_paged_kv8_op(q_out, k_pool, v_pool, k_scale, v_scale, block_table, cu_tokens, start_pos, scale, max_len,
                                         return_fp16)
    else:
        out = _prefill_attention_paged_impl(q_out, k_pool, v_pool, block_table, cu_tokens, start_pos, scale, max_len, return_fp16, k_scale,
                                            v_scale)
    return out if return_fp16 else out[:2]


# ---- the verify chunk's attention (include/qqq_amd_verify.h): `tokens` consecutive tokens per row through the decode kernel's operand
# layout, every token bit for bit decode_attention_paged(_kv8) of that token alone.

def _verify_attention_paged_shapes(name, q_out, k_pool, block_table, start, tokens, max_len):
    # (b, t, h, kvh, d, num_blocks, block_size, table_stride, max_len) from the tensors' shapes
    if k_pool.dim() != 4:
        raise RuntimeError(f"{name}: k_pool must be [num_blocks, kvh, block_size, d]")
    nb, kvh, bs, d = k_pool.shape
    if block_table.dim() != 2:
        raise RuntimeError(f"{name}: block_table must be int32 [b, blocks per row]")
    b, width = block_table.shape
    t = int(tokens)
    if t < 1:
        raise RuntimeError(f"{name}: tokens = {t}, need at least one token per row")
    if q_out.dim() != 3 or q_out.shape[0] != b * t or q_out.shape[2] != d:
        raise RuntimeError(f"{name}: q_out {tuple(q_out.shape)} must be [{b * t}, h, {d}] (rope_qkv_paged's output of {b} rows of {t} tokens)")
    if start.numel() != b:
        raise RuntimeError(f"{name}: start holds {start.numel()} positions, the block table has {b} rows")
    max_len = width * bs if max_len is None else int(max_len)
    return b, t, q_out.shape[1], kvh, d, nb, bs, width, max_len


def _verify_attention_paged_impl(q_out, k_pool, v_pool, block_table, start, tokens, scale, max_len, return_fp16, k_scale=None, v_scale=None):
    kv8 = k_scale is not None
    name = "verify_attention_paged_kv8" if kv8 else "verify_attention_paged"
    ts = (q_out, k_pool, v_pool, block_table, start) + ((k_scale, v_scale) if kv8 else ())
    _same_gpu(name, ts)
    if q_out.dtype != torch.float16 or start.dtype != torch.int64 or block_table.dtype != torch.int32:
        raise RuntimeError(f"{name}: q_out must be fp16, start int64 and block_table int32")
    _paged_check_pools(name, k_pool, v_pool, k_scale, v_scale)
    b, t, h, kvh, d, nb, bs, width, max_len = _verify_attention_paged_shapes(name, q_out, k_pool, block_table, start, tokens, max_len)
    dev = q_out.device
    m = b * t
    xq = torch.empty((m, h * d), dtype=torch.int8, device=dev)
    s1 = torch.empty((m, 1), dtype=torch.float32, device=dev)
    o16 = torch.empty((m, h * d) if return_fp16 else (0,), dtype=torch.float16, device=dev)
    if b == 0:
        return xq, s1, o16
    L = _lib.lib()
    nbytes = L.qqq_verify_attn_workspace_bytes(b, t, h, kvh, d, max_len)
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)  # torch's allocator: also under stream / graph capture
    q2, start, table = q_out.contiguous(), start.contiguous(), block_table.contiguous()
    tail = (_ptr(table), width, _ptr(start), float(scale), _ptr(o16), _ptr(xq), _ptr(s1), _ptr(ws), ws.numel(), b, t, h, kvh, d, nb, bs,
            max_len, dev.index or 0, _stream_for(q_out))
    if kv8:
        err = L.qqq_verify_attn_paged_kv8(_ptr(q2), _ptr(k_pool), _ptr(v_pool), _ptr(k_scale), _ptr(v_scale), *tail)
    else:
        err = L.qqq_verify_attn_paged(_ptr(q2), _ptr(k_pool), _ptr(v_pool), *tail)
    _raise_lib(name, err)
    return xq, s1, o16


def _verify_paged_fake(name, q_out, k_pool, block_table, start, tokens, max_len, return_fp16):
    b, t, h, _, d = _verify_attention_paged_shapes(name, q_out, k_pool, block_table, start, tokens, max_len)[:5]
    return (q_out.new_empty((b * t, h * d), dtype=torch.int8), q_out.new_empty((b * t, 1), dtype=torch.float32),
            q_out.new_empty((b * t, h * d) if return_fp16 else (0,), dtype=torch.float16))


@torch.library.custom_op("qqq_amd::verify_attn_paged", mutates_args=())
def _verify_attn_paged_op(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor, start: torch.Tensor,
                          tokens: int, scale: float, max_len: Optional[int],
                          return_fp16: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _verify_attention_paged_impl(q_out, k_pool, v_pool, block_table, start, tokens, scale, max_len, return_fp16)


@_verify_attn_paged_op.register_fake
def _(q_out, k_pool, v_pool, block_table, start, tokens, scale, max_len, return_fp16):
    return _verify_paged_fake("verify_attention_paged", q_out, k_pool, block_table, start, tokens, max_len, return_fp16)


def verify_attention_paged(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor, start: torch.Tensor,
                           tokens: int, scale: float, max_len: Optional[int] = None, return_fp16: bool = False):
    """Attention of a verify chunk -- `tokens` consecutive tokens per row, as a speculative decode step feeds them -- over a block pool:
    (xq int8 [b*tokens, h*d], s1 f32 [b*tokens, 1]), plus the fp16 output [b*tokens, h*d] with `return_fp16`.  Every token's rows are bit
    for bit decode_attention_paged's for that token alone (its q rows, pos = start + j, equal b and max_len); K and V are read once per KV
    head for the whole chunk and the keys stay split over workgroups.  Two launches.

    q_out      fp16 [b*tokens, h, d], token-major: rope_qkv_paged's output of the chunk (token j of row r is row r*tokens + j; the chunk's
               own keys are in the pool already)
    k_pool, v_pool, block_table   as for decode_attention_paged; only the entries up to (start[r] + tokens - 1) // block_size are read
    start      int64 [b]: the position of row r's first token; token j attends keys 0 ... start[r] + j
    tokens     1 ... 16, with (h / kvh) * tokens <= 64 and b * tokens <= 65535
    max_len    default and upper bound W * block_size; token j of a row with start[r] < 0 or start[r] + j >= max_len writes nothing (its
               rows are left as torch.empty made them)"""
    if _compiling(q_out, k_pool, v_pool, block_table, start):
        out = _verify_attn_paged_op(q_out, k_pool, v_pool, block_table, start, tokens, scale, max_len, return_fp16)
    else:
        out = _verify_attention_paged_impl(q_out, k_pool, v_pool, block_table, start, tokens, scale, max_len, return_fp16)
    return out if return_fp16 else out[:2]


@torch.library.custom_op("qqq_amd::verify_attn_paged_kv8", mutates_args=())
def _verify_attn_paged_kv8_op(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                              block_table: torch.Tensor, start: torch.Tensor, tokens: int, scale: float, max_len: Optional[int],
                              return_fp16: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _verify_attention_paged_impl(q_out, k_pool, v_pool, block_table, start, tokens, scale, max_len, return_fp16, k_scale, v_scale)


@_verify_attn_paged_kv8_op.register_fake
def _(q_out, k_pool, v_pool, k_scale, v_scale, block_table, start, tokens, scale, max_len, return_fp16):
    return _verify_paged_fake("verify_attention_paged_kv8", q_out, k_pool, block_table, start, tokens, max_len, return_fp16)


def verify_attention_paged_kv8(q_out: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                               block_table: torch.Tensor, start: torch.Tensor, tokens: int, scale: float, max_len: Optional[int] = None,
                               return_fp16: bool = False):
    """verify_attention_paged over an int8 pool (k_pool, v_pool int8 [num_blocks, kvh, block_size, d]; k_scale, v_scale f32 [num_blocks, kvh,
    block_size]): every token bit for bit decode_attention_paged_kv8's."""
    if _compiling(q_out, k_pool, v_pool, k_scale, v_scale, block_table, start):
        out = _verify_attn_paged_kv8_op(q_out, k_pool, v_pool, k_scale, v_scale, block_table, start, tokens, scale, max_len, return_fp16)
    else:
        out = _verify_attention_paged_impl(q_out, k_pool, v_pool, block_table, start, tokens, scale, max_len, return_fp16, k_scale, v_scale)
    return out if return_fp16 else out[:2]


# ---- the fused token sampler (include/qqq_amd_sample.h): logits -> next-token ids, one launch for the whole batch

def _sample_param(name, v, rows, dtype, device, op="sample_tokens"):
    # a per-row parameter: a tensor of `rows` entries on the logits' device, or a Python scalar that is broadcast
    if isinstance(v, torch.Tensor):
        if v.numel() != rows and v.numel() != 1:
            raise RuntimeError(f"{op}: {name} holds {v.numel()} entries, the logits have {rows} rows")
        if v.device != device:
            raise RuntimeError(f"{op}: {name} must be on the logits' device")
        v = v.reshape(-1).to(dtype)
        return (v.expand(rows) if v.numel() != rows else v).contiguous()
    return torch.full((rows,), v, dtype=dtype, device=device)


def _logits_rows(logits, vocab):
    # a row-strided view (the first vocab columns of a padded head output) is taken in place; anything else is copied into such rows
    if logits.stride(1) != 1 or logits.stride(0) < vocab or logits.stride(0) % 8 or logits.data_ptr() % 16:
        rows8 = torch.empty((logits.shape[0], vocab + (-vocab) % 8), dtype=torch.float16, device=logits.device)
        rows8[:, :vocab] = logits
        logits = rows8[:, :vocab]
    return logits


def _sample_tokens_impl(logits, temperature, top_k, top_p, u):
    ts = (logits, temperature, top_k, top_p, u)
    _same_gpu("sample_tokens", ts)
    if logits.dtype != torch.float16 or logits.dim() != 2:
        raise RuntimeError("sample_tokens: logits must be fp16 [rows, vocab]")
    rows, vocab = logits.shape
    if temperature.dtype != torch.float32 or top_p.dtype != torch.float32 or u.dtype != torch.float32 or top_k.dtype != torch.int32:
        raise RuntimeError("sample_tokens: temperature, top_p and u must be f32, top_k int32")
    if any(t.numel() != rows for t in ts[1:]):
        raise RuntimeError(f"sample_tokens: temperature, top_k, top_p and u must hold one entry per row ({rows})")
    if vocab < 1 or vocab > 262144 or rows > 65535:
        raise RuntimeError(f"sample_tokens: logits {tuple(logits.shape)} outside 1 <= vocab <= 262144, rows <= 65535")
    tokens = torch.empty((rows,), dtype=torch.int64, device=logits.device)
    if rows == 0:
        return tokens
    logits = _logits_rows(logits, vocab)
    err = _lib.lib().qqq_sample_tokens(_ptr(logits), logits.stride(0), _ptr(temperature.contiguous()), _ptr(top_k.contiguous()),
                                       _ptr(top_p.contiguous()), _ptr(u.contiguous()), _ptr(tokens), rows, vocab,
                                       logits.device.index or 0, _stream_for(logits))
    _raise_lib("sample_tokens", err)
    return tokens


@torch.library.custom_op("qqq_amd::sample_tokens", mutates_args=())
def _sample_tokens_op(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                      u: torch.Tensor) -> torch.Tensor:
    return _sample_tokens_impl(logits, temperature, top_k, top_p, u)


@_sample_tokens_op.register_fake
def _(logits, temperature, top_k, top_p, u):
    return logits.new_empty((logits.shape[0],), dtype=torch.int64)


def sample_tokens(logits: torch.Tensor, temperature, top_k, top_p, u: torch.Tensor) -> torch.Tensor:
    """The next token of every row of fp16 logits [rows, vocab]: temperature, top-k, top-p and the draw in one launch -> int64 [rows].

    temperature  f32 [rows] or a float: <= 0 (or NaN) is greedy, the lowest index of the maximum
    top_k        int32 [rows] or an int: <= 0 or >= vocab keeps every token, 1 is greedy; ties at the k-th largest value all stay
    top_p        f32 [rows] or a float: >= 1 keeps the top-k set; equal logits at the cut stay or go together
    u            f32 [rows]: one uniform variate in [0, 1) per row (torch.rand); the op holds no random state of its own
    The exact semantics of a row are stated in include/qqq_amd_sample.h.  Nothing is read on the host and the launch size depends on the
    shape alone, so a captured graph replays with other contents.  A view whose rows are `vocab` columns of a wider, 16-byte aligned
    fp16 matrix (row stride a multiple of 8) is read in place; its other columns are never touched."""
    if not isinstance(logits, torch.Tensor) or not isinstance(u, torch.Tensor) or logits.dim() != 2:
        raise RuntimeError("sample_tokens: logits must be an fp16 [rows, vocab] tensor and u an f32 [rows] tensor")
    rows, dev = logits.shape[0], logits.device
    temperature = _sample_param("temperature", temperature, rows, torch.float32, dev)
    top_k = _sample_param("top_k", top_k, rows, torch.int32, dev)
    top_p = _sample_param("top_p", top_p, rows, torch.float32, dev)
    if _compiling(logits, temperature, top_k, top_p, u):
        return _sample_tokens_op(logits, temperature, top_k, top_p, u)
    return _sample_tokens_impl(logits, temperature, top_k, top_p, u)


# ---- the fused scoring kernel (include/qqq_amd_score.h): logits + targets -> the targets' log-probabilities and the argmax, one launch

def _token_logprobs_check(logits, targets):
    if logits.dtype != torch.float16 or logits.dim() != 2:
        raise RuntimeError("token_logprobs: logits must be fp16 [rows, vocab]")
    rows, vocab = logits.shape
    if targets.dtype != torch.int64 or targets.dim() != 1 or targets.shape[0] != rows:
        raise RuntimeError(f"token_logprobs: targets must be int64 [{rows}], one entry per row, not {_dt(targets.dtype)} {tuple(targets.shape)}")
    if vocab < 1 or vocab > 262144 or rows > 1048576:
        raise RuntimeError(f"token_logprobs: logits {tuple(logits.shape)} outside 1 <= vocab <= 262144, rows <= 1048576")
    return rows, vocab


def _token_logprobs_impl(logits, targets, return_argmax):
    if not (logits.is_cuda and targets.is_cuda):
        raise RuntimeError("token_logprobs: logits and targets must be on the GPU (there is no CPU path)")
    if targets.device != logits.device:
        raise RuntimeError("token_logprobs: logits and targets must be on the same GPU")
    rows, vocab = _token_logprobs_check(logits, targets)
    logprob = torch.empty((rows,), dtype=torch.float32, device=logits.device)
    argmax = torch.empty((rows if return_argmax else 0,), dtype=torch.int64, device=logits.device)
    if rows == 0:
        return logprob, argmax
    logits = _logits_rows(logits, vocab)
    err = _lib.lib().qqq_token_logprobs(_ptr(logits), logits.stride(0), _ptr(targets.contiguous()), _ptr(logprob), _ptr(argmax), rows, vocab,
                                        logits.device.index or 0, _stream_for(logits))
    _raise_lib("token_logprobs", err)
    return logprob, argmax


@torch.library.custom_op("qqq_amd::token_logprobs", mutates_args=())
def _token_logprobs_op(logits: torch.Tensor, targets: torch.Tensor, return_argmax: bool) -> tuple[torch.Tensor, torch.Tensor]:
    return _token_logprobs_impl(logits, targets, return_argmax)


@_token_logprobs_op.register_fake
def _(logits, targets, return_argmax):
    rows, _ = _token_logprobs_check(logits, targets)
    return logits.new_empty((rows,), dtype=torch.float32), logits.new_empty((rows if return_argmax else 0,), dtype=torch.int64)


def token_logprobs(logits: torch.Tensor, targets: torch.Tensor, return_argmax: bool = True):
    """log softmax(logits[r])[targets[r]] for every row of fp16 logits [rows, vocab] and int64 targets [rows], in one launch and without an
    fp32 copy of the logits -> (logprob f32 [rows], argmax int64 [rows]; None with return_argmax=False).

    The exact semantics of a row are stated in include/qqq_amd_score.h: the weights are the sampler's at temperature 1 (fixed point, summed
    as integers, so a row's result is reproducible to the bit wherever the row sits), the logarithm is taken in f64 and rounded once;
    argmax is the token sample_tokens returns at temperature 0.  targets < 0 are ignored (logprob 0.0, as ignore_index), targets >= vocab
    give NaN, a target whose logit is NaN or -inf gives -inf.  Nothing is read on the host and the launch size depends on the shape alone,
    so a captured graph replays with other contents.  A view whose rows are `vocab` columns of a wider, 16-byte aligned fp16 matrix (row
    stride a multiple of 8) is read in place; its other columns are never touched."""
    if not isinstance(logits, torch.Tensor) or not isinstance(targets, torch.Tensor) or logits.dim() != 2:
        raise RuntimeError("token_logprobs: logits must be an fp16 [rows, vocab] tensor and targets an int64 [rows] tensor")
    return_argmax = bool(return_argmax)
    if _compiling(logits, targets):
        logprob, argmax = _token_logprobs_op(logits, targets, return_argmax)
    elif _ext() is not None:
        logprob, argmax = _EXT.token_logprobs(logits, targets, return_argmax)
    else:
        logprob, argmax = _token_logprobs_impl(logits, targets, return_argmax)
    return logprob, (argmax if return_argmax else None)


# ---- the decode loop's sample-and-advance step (include/qqq_amd_step.h): sample_tokens with an epilogue that advances every row's state

_ADVANCE_STATE = (("tick", torch.int32), ("ids", torch.int64), ("pos", torch.int64), ("slots", torch.int64), ("remaining", torch.int32),
                  ("eos", torch.int32), ("n_out", torch.int32))


# The checks of sample_advance and spec_advance that need no device -- dtypes and shapes, shared by the launch and the fake implementation
# -- are three helpers, called in the order the checks have always run in (an input with several faults reports the first): between them
# each op checks what it alone has.

def _sampler_inputs_check(op, logits, temperature, top_k, top_p, u, ids=None):
    # logits, the sampler's parameters and u -> (rows, group, vocab); `ids`: spec_advance's [rows, group], None: a logits row per row
    spec = ids is not None
    if logits.dtype != torch.float16 or logits.dim() != 2:
        raise RuntimeError(f"{op}: logits must be fp16 [{'rows * (draft_len + 1)' if spec else 'rows'}, vocab]")
    m, vocab = logits.shape
    rows, group = m, 1
    if spec:
        if ids.dtype != torch.int64 or ids.dim() != 2 or ids.shape[1] < 2 or ids.shape[1] > 16:
            raise RuntimeError(f"{op}: ids must be int64 [rows, draft_len + 1] with 1 <= draft_len <= 15, not {_dt(ids.dtype)} "
                               f"{tuple(ids.shape)}")
        rows, group = ids.shape
        if m != rows * group:
            raise RuntimeError(f"{op}: logits hold {m} rows, ids {tuple(ids.shape)} asks for {rows * group}")
    if temperature.dtype != torch.float32 or top_p.dtype != torch.float32 or u.dtype != torch.float32 or top_k.dtype != torch.int32:
        raise RuntimeError(f"{op}: temperature, top_p and u must be f32, top_k int32")
    if any(t.numel() != m for t in (temperature, top_k, top_p)):
        raise RuntimeError(f"{op}: temperature, top_k and top_p must hold one entry per {'logits row' if spec else 'row'} ({m})")
    if u.dim() != 2 or u.shape[0] != rows or u.shape[1] < group:
        raise RuntimeError(f"{op}: u must be f32 [{rows}, u_stride] with u_stride >= {f'draft_len + 1 = {group}' if spec else 1}, not "
                           f"{tuple(u.shape)}")
    return rows, group, vocab


def _row_state_check(op, rows, table, state, block_table):
    # the arrays that hold one entry per row, as `table` (_ADVANCE_STATE, _SPEC_ROW_STATE) lists them, and the block table
    for name, dtype in table:
        t = state[name]
        if t.dtype != dtype or t.dim() != 1 or t.shape[0] != rows:
            raise RuntimeError(f"{op}: {name} must be {_dt(dtype)} [{rows}], not {_dt(t.dtype)} {tuple(t.shape)}")
    if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != rows or block_table.shape[1] < 1:
        raise RuntimeError(f"{op}: block_table must be int32 [{rows}, blocks per row >= 1], not {tuple(block_table.shape)}")


def _sampler_limits_check(op, logits, block_size, ngram_max=None):
    # `ngram_max`: spec_advance's, whose logits hold draft_len + 1 rows per row
    if block_size not in (16, 32, 64, 128, 256):
        raise RuntimeError(f"{op}: block_size must be a power of two in [16, 256], not {block_size}")
    if ngram_max is not None and (ngram_max < 1 or ngram_max > 4):
        raise RuntimeError(f"{op}: ngram_max must be in [1, 4], not {ngram_max}")
    if logits.shape[1] < 1 or logits.shape[1] > 262144 or logits.shape[0] > 65535:
        raise RuntimeError(f"{op}: logits {tuple(logits.shape)} outside 1 <= vocab <= 262144, "
                           f"{'rows' if ngram_max is None else 'rows * (draft_len + 1)'} <= 65535")


def _in_place_check(op, named):
    # everything written is written in place: no copy may stand in for a state array
    for name, t in named:
        if not t.is_contiguous():
            raise RuntimeError(f"{op}: {name} must be contiguous (the state is updated in place)")


def _sample_advance_check(logits, temperature, top_k, top_p, u, tick, ids, pos, slots, block_table, remaining, eos, out, n_out, block_size):
    rows, _, vocab = _sampler_inputs_check("sample_advance", logits, temperature, top_k, top_p, u)
    _row_state_check("sample_advance", rows, _ADVANCE_STATE,
                     dict(tick=tick, ids=ids, pos=pos, slots=slots, remaining=remaining, eos=eos, n_out=n_out), block_table)
    if out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != rows or out.shape[1] < 1:
        raise RuntimeError(f"sample_advance: out must be int64 [{rows}, out_stride >= 1], not {tuple(out.shape)}")
    _sampler_limits_check("sample_advance", logits, block_size)
    return rows, vocab


def _sample_advance_impl(logits, temperature, top_k, top_p, u, tick, ids, pos, slots, block_table, remaining, eos, out, n_out, block_size):
    ts = (logits, temperature, top_k, top_p, u, tick, ids, pos, slots, block_table, remaining, eos, out, n_out)
    _same_gpu("sample_advance", ts)
    rows, vocab = _sample_advance_check(*ts, block_size)
    if rows == 0:
        return
    _in_place_check("sample_advance", (("u", u), ("tick", tick), ("ids", ids), ("pos", pos), ("slots", slots), ("block_table", block_table),
                                       ("remaining", remaining), ("eos", eos), ("out", out), ("n_out", n_out)))
    logits = _logits_rows(logits, vocab)
    err = _lib.lib().qqq_sample_advance(_ptr(logits), logits.stride(0), _ptr(temperature.contiguous()), _ptr(top_k.contiguous()),
                                        _ptr(top_p.contiguous()), _ptr(u), u.shape[1], _ptr(tick), _ptr(ids), _ptr(pos), _ptr(slots),
                                        _ptr(block_table), block_table.shape[1], _ptr(remaining), _ptr(eos), _ptr(out), out.shape[1],
                                        _ptr(n_out), rows, vocab, block_size, logits.device.index or 0, _stream_for(logits))
    _raise_lib("sample_advance", err)


@torch.library.custom_op("qqq_amd::sample_advance", mutates_args=("tick", "ids", "pos", "slots", "remaining", "out", "n_out"))
def _sample_advance_op(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor, u: torch.Tensor,
                       tick: torch.Tensor, ids: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor, block_table: torch.Tensor,
                       remaining: torch.Tensor, eos: torch.Tensor, out: torch.Tensor, n_out: torch.Tensor, block_size: int) -> None:
    _sample_advance_impl(logits, temperature, top_k, top_p, u, tick, ids, pos, slots, block_table, remaining, eos, out, n_out, block_size)


@_sample_advance_op.register_fake
def _(logits, temperature, top_k, top_p, u, tick, ids, pos, slots, block_table, remaining, eos, out, n_out, block_size):
    _sample_advance_check(logits, temperature, top_k, top_p, u, tick, ids, pos, slots, block_table, remaining, eos, out, n_out, block_size)


def sample_advance(logits: torch.Tensor, temperature, top_k, top_p, u: torch.Tensor, tick: torch.Tensor, ids: torch.Tensor,
                   pos: torch.Tensor, slots: torch.Tensor, block_table: torch.Tensor, remaining: torch.Tensor, eos: torch.Tensor,
                   out: torch.Tensor, n_out: torch.Tensor, block_size: int) -> None:
    """One decode step's sampling and bookkeeping in one launch: sample_tokens on every row of fp16 logits [rows, vocab], then -- on the
    device -- record the token, check eos and budget, and move the row to its next position and cache slot, or retire it.  Returns nothing;
    tick, ids, pos, slots, remaining, out and n_out are updated in place.

    temperature, top_k, top_p   as for sample_tokens (a tensor per row or a scalar)
    u            f32 [rows, u_stride]: row r draws with u[r, tick[r] % u_stride];  tick  int32 [rows], + 1 per call for every row
    ids, pos, slots   int64 [rows]: the next step's input token, its position (-1: an idle row) and its cache slot (-1 when idle)
    block_table  int32 [rows, W], only read;  block_size  the pool's (a power of two in [16, 256])
    remaining    int32 [rows]: tokens the row may still emit, 0 for an idle row;  eos  int32 [rows]: the row's eos id, -1 for none
    out          int64 [rows, out_stride], n_out int32 [rows]: the emitted tokens and their number
    A row that draws its eos, uses up its budget, or would leave its block table or out retires: ids 0, pos -1, slots -1, remaining 0.  The
    exact semantics of a row are stated in include/qqq_amd_step.h.  Nothing is read on the host and the launch size depends on the shape
    alone, so a decode step that ends in this call replays from a captured graph while rows finish and join."""
    if not isinstance(logits, torch.Tensor) or not isinstance(u, torch.Tensor) or logits.dim() != 2:
        raise RuntimeError("sample_advance: logits must be an fp16 [rows, vocab] tensor and u an f32 [rows, u_stride] tensor")
    rows, dev = logits.shape[0], logits.device
    temperature = _sample_param("temperature", temperature, rows, torch.float32, dev, "sample_advance")
    top_k = _sample_param("top_k", top_k, rows, torch.int32, dev, "sample_advance")
    top_p = _sample_param("top_p", top_p, rows, torch.float32, dev, "sample_advance")
    args = (logits, temperature, top_k, top_p, u, tick, ids, pos, slots, block_table, remaining, eos, out, n_out)
    if _compiling(*args):
        return _sample_advance_op(*args, int(block_size))
    return _sample_advance_impl(*args, int(block_size))


# ---- the speculative decode loop's verify-and-advance step (include/qqq_amd_spec.h): draft_len + 1 draws per row, the accept rule, the
# n-gram drafter and the next step's positions, on the device

_SPEC_ROW_STATE = (("tick", torch.int32), ("start", torch.int64), ("remaining", torch.int32), ("eos", torch.int32), ("hist_len", torch.int32),
                   ("n_out", torch.int32), ("n_acc", torch.int32))


def _spec_advance_check(logits, temperature, top_k, top_p, u, tick, ids, pos, slots, start, block_table, remaining, eos, hist, hist_len,
                        n_out, n_acc, block_size, ngram_max):
    rows, group, vocab = _sampler_inputs_check("spec_advance", logits, temperature, top_k, top_p, u, ids)
    for name, t in (("pos", pos), ("slots", slots)):
        if t.dtype != torch.int64 or tuple(t.shape) != (rows, group):
            raise RuntimeError(f"spec_advance: {name} must be int64 [{rows}, {group}], not {_dt(t.dtype)} {tuple(t.shape)}")
    _row_state_check("spec_advance", rows, _SPEC_ROW_STATE,
                     dict(tick=tick, start=start, remaining=remaining, eos=eos, hist_len=hist_len, n_out=n_out, n_acc=n_acc), block_table)
    if hist.dtype != torch.int32 or hist.dim() != 2 or hist.shape[0] != rows or hist.shape[1] < 1:
        raise RuntimeError(f"spec_advance: hist must be int32 [{rows}, hist_stride >= 1], not {_dt(hist.dtype)} {tuple(hist.shape)}")
    _sampler_limits_check("spec_advance", logits, block_size, ngram_max)
    return rows, group, vocab


def _spec_advance_impl(logits, temperature, top_k, top_p, u, tick, ids, pos, slots, start, block_table, remaining, eos, hist, hist_len,
                       n_out, n_acc, block_size, ngram_max):
    ts = (logits, temperature, top_k, top_p, u, tick, ids, pos, slots, start, block_table, remaining, eos, hist, hist_len, n_out, n_acc)
    _same_gpu("spec_advance", ts)
    rows, group, vocab = _spec_advance_check(*ts, block_size, ngram_max)
    if rows == 0:
        return
    _in_place_check("spec_advance", (("u", u), ("tick", tick), ("ids", ids), ("pos", pos), ("slots", slots), ("start", start),
                                     ("block_table", block_table), ("remaining", remaining), ("eos", eos), ("hist", hist),
                                     ("hist_len", hist_len), ("n_out", n_out), ("n_acc", n_acc)))
    logits = _logits_rows(logits, vocab)
    L = _lib.lib()
    ws = torch.empty((max(L.qqq_spec_advance_workspace_bytes(rows, group - 1), 16),), dtype=torch.uint8, device=logits.device)
    err = L.qqq_spec_advance(_ptr(logits), logits.stride(0), _ptr(temperature.contiguous()), _ptr(top_k.contiguous()),
                             _ptr(top_p.contiguous()), _ptr(u), u.shape[1], _ptr(tick), _ptr(ids), _ptr(pos), _ptr(slots), _ptr(start),
                             _ptr(block_table), block_table.shape[1], _ptr(remaining), _ptr(eos), _ptr(hist), hist.shape[1], _ptr(hist_len),
                             _ptr(n_out), _ptr(n_acc), _ptr(ws), ws.numel(), rows, group - 1, ngram_max, vocab, block_size,
                             logits.device.index or 0, _stream_for(logits))
    _raise_lib("spec_advance", err)


@torch.library.custom_op("qqq_amd::spec_advance",
                         mutates_args=("tick", "ids", "pos", "slots", "start", "remaining", "hist", "hist_len", "n_out", "n_acc"))
def _spec_advance_op(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor, u: torch.Tensor,
                     tick: torch.Tensor, ids: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor, start: torch.Tensor,
                     block_table: torch.Tensor, remaining: torch.Tensor, eos: torch.Tensor, hist: torch.Tensor, hist_len: torch.Tensor,
                     n_out: torch.Tensor, n_acc: torch.Tensor, block_size: int, ngram_max: int) -> None:
    _spec_advance_impl(logits, temperature, top_k, top_p, u, tick, ids, pos, slots, start, block_table, remaining, eos, hist, hist_len, n_out,
                       n_acc, block_size, ngram_max)


@_spec_advance_op.register_fake
def _(logits, temperature, top_k, top_p, u, tick, ids, pos, slots, start, block_table, remaining, eos, hist, hist_len, n_out, n_acc,
      block_size, ngram_max):
    _spec_advance_check(logits, temperature, top_k, top_p, u, tick, ids, pos, slots, start, block_table, remaining, eos, hist, hist_len,
                        n_out, n_acc, block_size, ngram_max)


def spec_advance(logits: torch.Tensor, temperature, top_k, top_p, u: torch.Tensor, tick: torch.Tensor, ids: torch.Tensor, pos: torch.Tensor,
                 slots: torch.Tensor, start: torch.Tensor, block_table: torch.Tensor, remaining: torch.Tensor, eos: torch.Tensor,
                 hist: torch.Tensor, hist_len: torch.Tensor, n_out: torch.Tensor, n_acc: torch.Tensor, block_size: int,
                 ngram_max: int = 3) -> None:
    """One speculative decode step's sampling, verification, drafting and bookkeeping: a row fed its last token and K = draft_len drafts
    through one forward; here each of its G = K + 1 logits rows is sampled as by sample_tokens, the draws behind a rightly guessed prefix
    are emitted (1 ... G tokens), the next K drafts come from an n-gram lookup in the row's history, and the row moves to its next
    positions and cache slots or retires -- all on the device, in two launches.  Returns nothing; tick, ids, pos, slots, start, remaining,
    hist, hist_len, n_out and n_acc are updated in place.

    logits       fp16 [rows * G, vocab]: draw j of row r reads row r * G + j
    temperature, top_k, top_p   as for sample_tokens, per logits row (a tensor of rows * G entries or a scalar)
    u            f32 [rows, u_stride >= G]: draw j of row r uses u[r, (tick[r] * G + j) % u_stride];  tick  int32 [rows], + 1 per call
    ids, pos, slots   int64 [rows, G]: flattened, the next forward's input_ids, PagedStep.pos and PagedStep.slots (idle: 0, -1, -1)
    start        int64 [rows]: PagedStep.start_pos, = pos[:, 0];  block_table  int32 [rows, W], only read;  block_size  the pool's
    remaining    int32 [rows]: tokens the row may still emit, 0 for an idle row;  eos  int32 [rows]: the row's eos id, -1 for none
    hist         int32 [rows, hist_stride], hist_len int32 [rows]: the sequence so far, prompt and emitted tokens
    n_out, n_acc int32 [rows]: tokens emitted (they are hist[r, hist_len - n_out : hist_len]) and drafts accepted since last cleared
    ngram_max    the longest n-gram the drafter looks up, 1 ... 4
    Every emitted token is a plain sampler draw from logits computed on the true prefix, so the output distribution is the sampler's at any
    temperature, top_k and top_p.  The exact semantics of a row are stated in include/qqq_amd_spec.h.  Nothing is read on the host and the
    launch sizes depend on the shapes alone, so a step that ends in this call replays from a captured graph while rows finish and join."""
    if not isinstance(logits, torch.Tensor) or not isinstance(u, torch.Tensor) or not isinstance(ids, torch.Tensor) or logits.dim() != 2:
        raise RuntimeError("spec_advance: logits must be an fp16 [rows * (draft_len + 1), vocab] tensor, u an f32 [rows, u_stride] tensor "
                           "and ids an int64 [rows, draft_len + 1] tensor")
    m, dev = logits.shape[0], logits.device
    temperature = _sample_param("temperature", temperature, m, torch.float32, dev, "spec_advance")
    top_k = _sample_param("top_k", top_k, m, torch.int32, dev, "spec_advance")
    top_p = _sample_param("top_p", top_p, m, torch.float32, dev, "spec_advance")
    args = (logits, temperature, top_k, top_p, u, tick, ids, pos, slots, start, block_table, remaining, eos, hist, hist_len, n_out, n_acc)
    if _compiling(*args):
        return _spec_advance_op(*args, int(block_size), int(ngram_max))
    return _spec_advance_impl(*args, int(block_size), int(ngram_max))


# ---- the repetition / presence / frequency penalty (include/qqq_amd_penalty.h): the logits rewritten in place from each row's history, in
# front of any of the three samplers above

_PENALTY_ROW_STATE = (("n_prompt", torch.int32), ("repetition_penalty", torch.float32), ("presence_penalty", torch.float32),
                      ("frequency_penalty", torch.float32))


def _penalize_logits_check(logits, ids, pos, seen, n_prompt, repetition_penalty, presence_penalty, frequency_penalty, workspace):
    # dtypes, shapes and strides: needs no device, shared by the launch and the fake implementation -> (rows, group, vocab)
    op = "penalize_logits"
    if logits.dtype != torch.float16 or logits.dim() != 2:
        raise RuntimeError(f"{op}: logits must be fp16 [rows * group, vocab]")
    m, vocab = logits.shape
    if ids.dtype != torch.int64 or ids.dim() not in (1, 2) or (ids.dim() == 2 and not 1 <= ids.shape[1] <= 16):
        raise RuntimeError(f"{op}: ids must be int64 [rows] or [rows, group] with 1 <= group <= 16, not {_dt(ids.dtype)} {tuple(ids.shape)}")
    rows, group = ids.shape[0], (ids.shape[1] if ids.dim() == 2 else 1)
    if m != rows * group:
        raise RuntimeError(f"{op}: logits hold {m} rows, ids {tuple(ids.shape)} asks for {rows * group}")
    if pos.dtype != torch.int64 or pos.shape != ids.shape:
        raise RuntimeError(f"{op}: pos must be int64 {tuple(ids.shape)} like ids, not {_dt(pos.dtype)} {tuple(pos.shape)}")
    if seen.dtype != torch.int32 or seen.dim() != 2 or seen.shape[0] != rows or seen.shape[1] < 1:
        raise RuntimeError(f"{op}: seen must be int32 [{rows}, seen_stride >= 1], not {_dt(seen.dtype)} {tuple(seen.shape)}")
    state = dict(n_prompt=n_prompt, repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                 frequency_penalty=frequency_penalty)
    for name, dtype in _PENALTY_ROW_STATE:
        t = state[name]
        if t.dtype != dtype or t.dim() != 1 or t.shape[0] != rows:
            raise RuntimeError(f"{op}: {name} must be {_dt(dtype)} [{rows}], not {_dt(t.dtype)} {tuple(t.shape)}")
    if workspace.dtype != torch.int32 or workspace.dim() != 1 or workspace.shape[0] < rows * vocab:
        raise RuntimeError(f"{op}: workspace must be int32 [>= rows * vocab = {rows * vocab}], zero on entry, not {_dt(workspace.dtype)} "
                           f"{tuple(workspace.shape)}")
    if vocab < 1 or vocab > 262144 or m > 65535 or seen.shape[1] >= 1 << 30:
        raise RuntimeError(f"{op}: logits {tuple(logits.shape)} outside 1 <= vocab <= 262144, rows * group <= 65535, or seen_stride "
                           f"{seen.shape[1]} >= 2^30")
    if m and (logits.stride(1) != 1 or logits.stride(0) < vocab):
        raise RuntimeError(f"{op}: logits must have unit column stride and a row stride >= vocab (they are rewritten in place, never "
                           f"copied), not strides {tuple(logits.stride())}")
    return rows, group, vocab


def _penalize_logits_impl(logits, ids, pos, seen, n_prompt, repetition_penalty, presence_penalty, frequency_penalty, workspace):
    ts = (logits, ids, pos, seen, n_prompt, repetition_penalty, presence_penalty, frequency_penalty, workspace)
    _same_gpu("penalize_logits", ts)
    rows, group, vocab = _penalize_logits_check(*ts)
    if rows == 0:
        return
    _in_place_check("penalize_logits", (("ids", ids), ("pos", pos), ("seen", seen), ("n_prompt", n_prompt),
                                        ("repetition_penalty", repetition_penalty), ("presence_penalty", presence_penalty),
                                        ("frequency_penalty", frequency_penalty), ("workspace", workspace)))
    err = _lib.lib().qqq_penalize_logits(_ptr(logits), logits.stride(0), _ptr(ids), _ptr(pos), group, _ptr(seen), seen.shape[1],
                                         _ptr(n_prompt), _ptr(repetition_penalty), _ptr(presence_penalty), _ptr(frequency_penalty),
                                         _ptr(workspace), workspace.numel() * 4, rows, vocab, logits.device.index or 0, _stream_for(logits))
    _raise_lib("penalize_logits", err)


@torch.library.custom_op("qqq_amd::penalize_logits", mutates_args=("logits", "seen", "workspace"))
def _penalize_logits_op(logits: torch.Tensor, ids: torch.Tensor, pos: torch.Tensor, seen: torch.Tensor, n_prompt: torch.Tensor,
                        repetition_penalty: torch.Tensor, presence_penalty: torch.Tensor, frequency_penalty: torch.Tensor,
                        workspace: torch.Tensor) -> None:
    _penalize_logits_impl(logits, ids, pos, seen, n_prompt, repetition_penalty, presence_penalty, frequency_penalty, workspace)


@_penalize_logits_op.register_fake
def _(logits, ids, pos, seen, n_prompt, repetition_penalty, presence_penalty, frequency_penalty, workspace):
    _penalize_logits_check(logits, ids, pos, seen, n_prompt, repetition_penalty, presence_penalty, frequency_penalty, workspace)


def penalize_logits(logits: torch.Tensor, ids: torch.Tensor, pos: torch.Tensor, seen: torch.Tensor, n_prompt: torch.Tensor,
                    repetition_penalty, presence_penalty, frequency_penalty, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Repetition, presence and frequency penalties on fp16 logits [rows * G, vocab], in place and in one launch, in front of
    sample_tokens, sample_advance or spec_advance -> `logits`.  logits, seen and the workspace are updated in place.

    ids, pos     int64 [rows] (G = 1) or [rows, G <= 16]: a loop's state arrays -- the tokens a row feeds through the forward (its last
                 token, then its drafts) and their positions, of which pos[r, 0] alone is read; < 0 (an idle row) or >= seen_stride: the
                 row is left alone altogether
    seen         int32 [rows, seen_stride]: the sequence so far.  The op records ids[r, 0] at seen[r, pos[r, 0]] itself
    n_prompt     int32 [rows]: the prompt's length; presence and frequency count the occurrences at indices >= n_prompt alone
    repetition_penalty, presence_penalty, frequency_penalty   f32 [rows] or a float: 1, 0 and 0 leave a row's logits alone
    workspace    int32 [>= rows * vocab], zero on entry and left zero (allocate once, reuse); None allocates a zeroed one
    Logits row r * G + j is conditioned on seen[r, :pos[r, 0] + 1] and the drafts ids[r, 1 ... j]: every token t in it takes
    l = l > 0 ? l / repetition : l * repetition (transformers' rule), then, with c > 0 occurrences among the outputs,
    l - frequency * c - presence (vLLM's); each step one f32 operation, the result rounded to fp16.  The exact semantics of a row are
    stated in include/qqq_amd_penalty.h.  Nothing is read on the host and the launch size depends on the shapes alone, so a step with this
    call in it replays from a captured graph.  The logits are never copied: unit column stride and a row stride >= vocab, or it raises."""
    if not isinstance(logits, torch.Tensor) or not isinstance(ids, torch.Tensor) or logits.dim() != 2 or ids.dim() not in (1, 2):
        raise RuntimeError("penalize_logits: logits must be an fp16 [rows * group, vocab] tensor and ids an int64 [rows] or [rows, group] "
                           "tensor")
    if not isinstance(repetition_penalty, torch.Tensor):
        repetition_penalty = float(repetition_penalty)
        if not (repetition_penalty > 0.0 and repetition_penalty != float("inf")):
            raise ValueError(f"penalize_logits: repetition_penalty={repetition_penalty} must be finite and > 0")
    rows, dev = ids.shape[0], logits.device
    repetition_penalty = _sample_param("repetition_penalty", repetition_penalty, rows, torch.float32, dev, "penalize_logits")
    presence_penalty = _sample_param("presence_penalty", presence_penalty, rows, torch.float32, dev, "penalize_logits")
    frequency_penalty = _sample_param("frequency_penalty", frequency_penalty, rows, torch.float32, dev, "penalize_logits")
    if workspace is None:
        workspace = torch.zeros((rows * logits.shape[1],), dtype=torch.int32, device=dev)
    args = (logits, ids, pos, seen, n_prompt, repetition_penalty, presence_penalty, frequency_penalty, workspace)
    if _compiling(*args):
        _penalize_logits_op(*args)
    else:
        _penalize_logits_impl(*args)
    return logits


# ---- the fused top-k log-probability kernel (include/qqq_amd_logprobs.h): the log-probability and rank of a token and the k most
# probable tokens of every logits row, one launch; behind a sampler, on the logits it drew from

def _topk_k_check(op, k, vocab):
    if k < 0 or k > 32 or k > vocab:
        raise ValueError(f"{op}: k={k} outside [0, min(32, vocab={vocab})]")


def _topk_logprobs_check(logits, tokens, k):
    # dtypes and shapes: needs no device, shared by the launch and the fake implementation -> (rows, vocab)
    op = "topk_logprobs"
    if logits.dtype != torch.float16 or logits.dim() != 2:
        raise RuntimeError(f"{op}: logits must be fp16 [rows, vocab]")
    rows, vocab = logits.shape
    if tokens is not None and (tokens.dtype != torch.int64 or tokens.dim() != 1 or tokens.shape[0] != rows):
        raise RuntimeError(f"{op}: tokens must be int64 [{rows}], one entry per row, not {_dt(tokens.dtype)} {tuple(tokens.shape)}")
    if vocab < 1 or vocab > 262144 or rows > 65535:
        raise RuntimeError(f"{op}: logits {tuple(logits.shape)} outside 1 <= vocab <= 262144, rows <= 65535")
    _topk_k_check(op, k, vocab)
    if tokens is None and k == 0:
        raise ValueError(f"{op}: nothing is asked for (tokens is None and k == 0)")
    return rows, vocab


def _topk_logprobs_outputs(like, rows, scored, k):
    return (like.new_empty((rows if scored else 0,), dtype=torch.float32), like.new_empty((rows if scored else 0,), dtype=torch.int32),
            like.new_empty((rows, k), dtype=torch.int32), like.new_empty((rows, k), dtype=torch.float32))


def _topk_logprobs_impl(logits, tokens, k):
    _same_gpu("topk_logprobs", (logits,) if tokens is None else (logits, tokens))
    rows, vocab = _topk_logprobs_check(logits, tokens, k)
    logprob, rank, top_ids, top_lp = _topk_logprobs_outputs(logits, rows, tokens is not None, k)
    if rows == 0:
        return logprob, rank, top_ids, top_lp
    logits = _logits_rows(logits, vocab)
    err = _lib.lib().qqq_topk_logprobs(_ptr(logits), logits.stride(0), None if tokens is None else _ptr(tokens.contiguous()), _ptr(logprob),
                                       _ptr(rank), _ptr(top_ids), _ptr(top_lp), k, rows, vocab, logits.device.index or 0,
                                       _stream_for(logits))
    _raise_lib("topk_logprobs", err)
    return logprob, rank, top_ids, top_lp


@torch.library.custom_op("qqq_amd::topk_logprobs", mutates_args=())
def _topk_logprobs_op(logits: torch.Tensor, tokens: Optional[torch.Tensor], k: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                                                                              torch.Tensor]:
    return _topk_logprobs_impl(logits, tokens, k)


@_topk_logprobs_op.register_fake
def _(logits, tokens, k):
    rows, _ = _topk_logprobs_check(logits, tokens, k)
    return _topk_logprobs_outputs(logits, rows, tokens is not None, k)


def topk_logprobs(logits: torch.Tensor, tokens: Optional[torch.Tensor] = None, k: int = 0):
    """For every row of fp16 logits [rows, vocab]: the log-probability and the rank of tokens[r] (int64 [rows]) under softmax(logits[r]),
    and the k most probable tokens with their log-probabilities, in one launch -> (logprob f32 [rows], rank int32 [rows], top_ids int32
    [rows, k], top_logprobs f32 [rows, k]); the first two are None with tokens=None, the last two with k=0.

    logprob is ops.token_logprobs' value to the bit (tokens < 0 give 0.0, tokens >= vocab NaN, a token whose logit is NaN or -inf
    -inf); rank is 1 + the number of logits above the token's (0 for a token outside [0, vocab)); the top-k entries are ordered by logit
    descending, then index ascending, with ties at the cut resolved exactly, and top_logprobs[r, i] is the value logprob has for
    top_ids[r, i]: entry 0 is sample_tokens' greedy token.  0 <= k <= min(32, vocab).  The exact semantics of a row are stated in
    include/qqq_amd_logprobs.h.  Nothing is read on the host and the launch size depends on (rows, vocab, k) alone, so a captured
    graph replays with other contents.  A view whose rows are `vocab` columns of a wider, 16-byte aligned fp16 matrix (row stride a
    multiple of 8) is read in place; its other columns are never touched."""
    if not isinstance(logits, torch.Tensor) or (tokens is not None and not isinstance(tokens, torch.Tensor)) or logits.dim() != 2:
        raise RuntimeError("topk_logprobs: logits must be an fp16 [rows, vocab] tensor and tokens an int64 [rows] tensor or None")
    k = int(k)
    if _compiling(logits, tokens):
        logprob, rank, top_ids, top_lp = _topk_logprobs_op(logits, tokens, k)
    else:
        logprob, rank, top_ids, top_lp = _topk_logprobs_impl(logits, tokens, k)
    scored = tokens is not None
    return (logprob if scored else None, rank if scored else None, top_ids if k else None, top_lp if k else None)


def _topk_logprobs_step_check(logits, out, n_out, n_rec, logprob, rank, top_ids, top_logprobs):
    # dtypes and shapes -> (rows, vocab, cap, k)
    op = "topk_logprobs_step"
    if logits.dtype != torch.float16 or logits.dim() != 2:
        raise RuntimeError(f"{op}: logits must be fp16 [rows, vocab]")
    rows, vocab = logits.shape
    if out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != rows or out.shape[1] < 1:
        raise RuntimeError(f"{op}: out must be int64 [{rows}, out_stride >= 1], not {_dt(out.dtype)} {tuple(out.shape)}")
    for name, t in (("n_out", n_out), ("n_rec", n_rec)):
        if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != rows:
            raise RuntimeError(f"{op}: {name} must be int32 [{rows}], not {_dt(t.dtype)} {tuple(t.shape)}")
    if logprob.dtype != torch.float32 or logprob.dim() != 2 or logprob.shape[0] != rows or logprob.shape[1] < 1:
        raise RuntimeError(f"{op}: logprob must be f32 [{rows}, cap >= 1], not {_dt(logprob.dtype)} {tuple(logprob.shape)}")
    cap = logprob.shape[1]
    if rank.dtype != torch.int32 or tuple(rank.shape) != (rows, cap):
        raise RuntimeError(f"{op}: rank must be int32 [{rows}, {cap}] like logprob, not {_dt(rank.dtype)} {tuple(rank.shape)}")
    if top_ids.dtype != torch.int32 or top_ids.dim() != 3 or tuple(top_ids.shape[:2]) != (rows, cap):
        raise RuntimeError(f"{op}: top_ids must be int32 [{rows}, {cap}, k], not {_dt(top_ids.dtype)} {tuple(top_ids.shape)}")
    k = top_ids.shape[2]
    if top_logprobs.dtype != torch.float32 or tuple(top_logprobs.shape) != (rows, cap, k):
        raise RuntimeError(f"{op}: top_logprobs must be f32 [{rows}, {cap}, {k}] like top_ids, not {_dt(top_logprobs.dtype)} "
                           f"{tuple(top_logprobs.shape)}")
    if vocab < 1 or vocab > 262144 or rows > 65535:
        raise RuntimeError(f"{op}: logits {tuple(logits.shape)} outside 1 <= vocab <= 262144, rows <= 65535")
    _topk_k_check(op, k, vocab)
    return rows, vocab, cap, k


def _topk_logprobs_step_impl(logits, out, n_out, n_rec, logprob, rank, top_ids, top_logprobs):
    ts = (logits, out, n_out, n_rec, logprob, rank, top_ids, top_logprobs)
    _same_gpu("topk_logprobs_step", ts)
    rows, vocab, cap, k = _topk_logprobs_step_check(*ts)
    if rows == 0:
        return
    _in_place_check("topk_logprobs_step", (("out", out), ("n_out", n_out), ("n_rec", n_rec), ("logprob", logprob), ("rank", rank),
                                           ("top_ids", top_ids), ("top_logprobs", top_logprobs)))
    logits = _logits_rows(logits, vocab)
    err = _lib.lib().qqq_topk_logprobs_step(_ptr(logits), logits.stride(0), _ptr(out), out.shape[1], _ptr(n_out), _ptr(n_rec), _ptr(logprob),
                                            _ptr(rank), _ptr(top_ids), _ptr(top_logprobs), cap, k, rows, vocab, logits.device.index or 0,
                                            _stream_for(logits))
    _raise_lib("topk_logprobs_step", err)


@torch.library.custom_op("qqq_amd::topk_logprobs_step", mutates_args=("n_rec", "logprob", "rank", "top_ids", "top_logprobs"))
def _topk_logprobs_step_op(logits: torch.Tensor, out: torch.Tensor, n_out: torch.Tensor, n_rec: torch.Tensor, logprob: torch.Tensor,
                           rank: torch.Tensor, top_ids: torch.Tensor, top_logprobs: torch.Tensor) -> None:
    _topk_logprobs_step_impl(logits, out, n_out, n_rec, logprob, rank, top_ids, top_logprobs)


@_topk_logprobs_step_op.register_fake
def _(logits, out, n_out, n_rec, logprob, rank, top_ids, top_logprobs):
    _topk_logprobs_step_check(logits, out, n_out, n_rec, logprob, rank, top_ids, top_logprobs)


def topk_logprobs_step(logits: torch.Tensor, out: torch.Tensor, n_out: torch.Tensor, n_rec: torch.Tensor, logprob: torch.Tensor,
                       rank: torch.Tensor, top_ids: Optional[torch.Tensor] = None, top_logprobs: Optional[torch.Tensor] = None) -> None:
    """The decode loop's log-probability epilogue, behind sample_advance on the logits that call drew from: a row that holds a token
    without a record yet gets topk_logprobs' results for it, in place.  Returns nothing; n_rec, logprob, rank, top_ids and top_logprobs
    are updated in place.

    out, n_out   int64 [rows, out_stride], int32 [rows]: sample_advance's emitted tokens and their number, only read
    n_rec        int32 [rows]: the records a row has so far
    logprob, rank             f32 / int32 [rows, cap];  top_ids, top_logprobs  int32 / f32 [rows, cap, k], or both None for k = 0
    A row with n_rec[r] < n_out[r] and n_rec[r] < cap scores out[r, n_rec[r]] against logits[r] into record (r, n_rec[r]) and counts it;
    every other row -- idle, nothing emitted in this step, no room -- writes nothing.  At most one record per row and call.  The exact
    semantics are stated in include/qqq_amd_logprobs.h.  Nothing is read on the host and the launch size depends on the shapes
    alone, so a decode step with this call behind sample_advance replays from a captured graph."""
    if not isinstance(logits, torch.Tensor) or not isinstance(logprob, torch.Tensor) or logits.dim() != 2 or logprob.dim() != 2:
        raise RuntimeError("topk_logprobs_step: logits must be an fp16 [rows, vocab] tensor and logprob an f32 [rows, cap] tensor")
    if (top_ids is None) != (top_logprobs is None):
        raise RuntimeError("topk_logprobs_step: top_ids and top_logprobs must be given or None together")
    if top_ids is None:  # k = 0: nothing of them is ever touched
        top_ids = logprob.new_empty(tuple(logprob.shape) + (0,), dtype=torch.int32)
        top_logprobs = logprob.new_empty(tuple(logprob.shape) + (0,))
    args = (logits, out, n_out, n_rec, logprob, rank, top_ids, top_logprobs)
    if _compiling(*args):
        return _topk_logprobs_step_op(*args)
    return _topk_logprobs_step_impl(*args)


# ---- stop sequences, stop token ids and the minimum length (include/qqq_amd_stop.h): the ban in front of a sampler, the
# check behind a decode loop's step

def _rows_i32_check(op, rows, named):
    for name, t in named:
        if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != rows:
            raise RuntimeError(f"{op}: {name} must be int32 [{rows}], not {_dt(t.dtype)} {tuple(t.shape)}")


def _id_list_check(op, name, t):
    if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] > 32:
        raise RuntimeError(f"{op}: {name} must be int32 [at most 32], not {_dt(t.dtype)} {tuple(t.shape)}")


def _ban_tokens_check(logits, n_out, min_new, eos, ban_ids, base):
    # dtypes, shapes and strides -> (rows, group, vocab)
    op = "ban_tokens"
    if logits.dtype != torch.float16 or logits.dim() != 2:
        raise RuntimeError(f"{op}: logits must be fp16 [rows * group, vocab]")
    m, vocab = logits.shape
    if n_out.dtype != torch.int32 or n_out.dim() != 1:
        raise RuntimeError(f"{op}: n_out must be int32 [rows], not {_dt(n_out.dtype)} {tuple(n_out.shape)}")
    rows = n_out.shape[0]
    group = m // rows if rows else 1
    if m != rows * group or not 1 <= group <= 16:
        raise RuntimeError(f"{op}: logits hold {m} rows, n_out {tuple(n_out.shape)} asks for rows * group with 1 <= group <= 16")
    _rows_i32_check(op, rows, (("min_new", min_new), ("eos", eos)))
    _id_list_check(op, "ban_ids", ban_ids)
    if vocab < 1 or vocab > 262144 or m > 65535:
        raise RuntimeError(f"{op}: logits {tuple(logits.shape)} outside 1 <= vocab <= 262144, rows * group <= 65535")
    if m and (logits.stride(1) != 1 or logits.stride(0) < vocab):
        raise RuntimeError(f"{op}: logits must have unit column stride and a row stride >= vocab (they are rewritten in place, never "
                           f"copied), not strides {tuple(logits.stride())}")
    return rows, group, vocab


def _ban_tokens_impl(logits, n_out, min_new, eos, ban_ids, base):
    ts = (logits, n_out, min_new, eos, ban_ids)
    _same_gpu("ban_tokens", ts)
    rows, group, vocab = _ban_tokens_check(*ts, base)
    if rows == 0:
        return
    _in_place_check("ban_tokens", (("n_out", n_out), ("min_new", min_new), ("eos", eos), ("ban_ids", ban_ids)))
    err = _lib.lib().qqq_ban_tokens(_ptr(logits), logits.stride(0), _ptr(n_out), base, _ptr(min_new), _ptr(eos), _ptr(ban_ids),
                                    ban_ids.shape[0], group, rows, vocab, logits.device.index or 0, _stream_for(logits))
    _raise_lib("ban_tokens", err)


@torch.library.custom_op("qqq_amd::ban_tokens", mutates_args=("logits",))
def _ban_tokens_op(logits: torch.Tensor, n_out: torch.Tensor, min_new: torch.Tensor, eos: torch.Tensor, ban_ids: torch.Tensor,
                   base: int) -> None:
    _ban_tokens_impl(logits, n_out, min_new, eos, ban_ids, base)


@_ban_tokens_op.register_fake
def _(logits, n_out, min_new, eos, ban_ids, base):
    _ban_tokens_check(logits, n_out, min_new, eos, ban_ids, base)


def ban_tokens(logits: torch.Tensor, n_out: torch.Tensor, min_new: torch.Tensor, eos: torch.Tensor,
               ban_ids: Optional[torch.Tensor] = None, base: int = 0) -> torch.Tensor:
    """The minimum length of a completion on fp16 logits [rows * G, vocab], in place and in one launch, in front of sample_tokens,
    sample_advance or spec_advance (behind penalize_logits) -> `logits`.

    n_out        int32 [rows]: the tokens a row has emitted;  base  an int added to it (the loops pass 1: n_out does not count the
                 prefill's token; admission and the host path pass 0 and their own counts)
    min_new      int32 [rows]: the row's minimum length;  eos  int32 [rows]: the row's eos id, -1 for none
    ban_ids      int32 [at most 32] or None: the stop token ids, shared by the rows
    Logits row r * G + j (G = logits rows / rows, at most 16) is the one the completion's token of index n_out[r] + base + j is drawn from:
    if that index is below min_new[r], the row's eos and every ban id become -inf there.  Ids outside [0, vocab) are ignored; every other
    entry keeps its bits.  The exact semantics are stated in include/qqq_amd_stop.h.  Nothing is read on the host and the
    launch size depends on the shapes alone, so a step with this call in it replays from a captured graph.  The logits are never
    copied: unit column stride and a row stride >= vocab, or it raises."""
    if not isinstance(logits, torch.Tensor) or not isinstance(n_out, torch.Tensor) or logits.dim() != 2 or n_out.dim() != 1:
        raise RuntimeError("ban_tokens: logits must be an fp16 [rows * group, vocab] tensor and n_out an int32 [rows] tensor")
    if ban_ids is None:
        ban_ids = n_out.new_empty((0,), dtype=torch.int32)
    args = (logits, n_out, min_new, eos, ban_ids, int(base))
    if _compiling(*args[:5]):
        _ban_tokens_op(*args)
    else:
        _ban_tokens_impl(*args)
    return logits


def _stop_check_check(tokens, base, first, n_out, stop_ids, stop_len, end_ids, eos, min_new, n_seen, n_trim, stop_hit, ids, pos, slots,
                      start, remaining):
    # dtypes and shapes -> (rows, group)
    op = "stop_check"
    if tokens.dtype not in (torch.int32, torch.int64) or tokens.dim() != 2 or tokens.shape[1] < 1:
        raise RuntimeError(f"{op}: tokens must be int32 or int64 [rows, stride >= 1], not {_dt(tokens.dtype)} {tuple(tokens.shape)}")
    rows = tokens.shape[0]
    if ids.dtype != torch.int64 or ids.dim() not in (1, 2) or ids.shape[0] != rows or (ids.dim() == 2 and not 1 <= ids.shape[1] <= 16):
        raise RuntimeError(f"{op}: ids must be int64 [{rows}] or [{rows}, group] with 1 <= group <= 16, not {_dt(ids.dtype)} {tuple(ids.shape)}")
    group = ids.shape[1] if ids.dim() == 2 else 1
    for name, t in (("pos", pos), ("slots", slots)):
        if t.dtype != torch.int64 or t.shape != ids.shape:
            raise RuntimeError(f"{op}: {name} must be int64 {tuple(ids.shape)} like ids, not {_dt(t.dtype)} {tuple(t.shape)}")
    if start is not None and (start.dtype != torch.int64 or start.dim() != 1 or start.shape[0] != rows):
        raise RuntimeError(f"{op}: start must be int64 [{rows}] or None, not {_dt(start.dtype)} {tuple(start.shape)}")
    named = [("base", base), ("n_out", n_out), ("min_new", min_new), ("n_seen", n_seen), ("n_trim", n_trim), ("stop_hit", stop_hit),
             ("remaining", remaining)] + ([("first", first)] if first is not None else []) + ([("eos", eos)] if eos is not None else [])
    _rows_i32_check(op, rows, named)
    if stop_ids.dtype != torch.int32 or stop_ids.dim() != 2 or stop_ids.shape[0] > 32 or not 1 <= stop_ids.shape[1] <= 32:
        raise RuntimeError(f"{op}: stop_ids must be int32 [n_stop <= 32, 1 <= stop_stride <= 32], not {_dt(stop_ids.dtype)} "
                           f"{tuple(stop_ids.shape)}")
    if stop_len.dtype != torch.int32 or tuple(stop_len.shape) != (stop_ids.shape[0],):
        raise RuntimeError(f"{op}: stop_len must be int32 [{stop_ids.shape[0]}], one entry per stop sequence, not {_dt(stop_len.dtype)} "
                           f"{tuple(stop_len.shape)}")
    _id_list_check(op, "end_ids", end_ids)
    if rows > 65535:
        raise RuntimeError(f"{op}: rows={rows} exceeds 65535")
    return rows, group


def _stop_check_impl(tokens, base, first, n_out, stop_ids, stop_len, end_ids, eos, min_new, n_seen, n_trim, stop_hit, ids, pos, slots,
                     start, remaining):
    args = (tokens, base, first, n_out, stop_ids, stop_len, end_ids, eos, min_new, n_seen, n_trim, stop_hit, ids, pos, slots, start,
            remaining)
    names = ("tokens", "base", "first", "n_out", "stop_ids", "stop_len", "end_ids", "eos", "min_new", "n_seen", "n_trim", "stop_hit", "ids",
             "pos", "slots", "start", "remaining")
    given = [(n, t) for n, t in zip(names, args) if t is not None]
    _same_gpu("stop_check", [t for _, t in given])
    rows, group = _stop_check_check(*args)
    if rows == 0:
        return
    _in_place_check("stop_check", given)
    err = _lib.lib().qqq_stop_check(_ptr(tokens), tokens.element_size(), tokens.shape[1], _ptr(base), _ptr(first), _ptr(n_out),
                                    _ptr(stop_ids), stop_ids.shape[1], _ptr(stop_len), stop_ids.shape[0], _ptr(end_ids), end_ids.shape[0],
                                    _ptr(eos), _ptr(min_new), _ptr(n_seen), _ptr(n_trim), _ptr(stop_hit), _ptr(ids), _ptr(pos), _ptr(slots), _ptr(start),
                                    _ptr(remaining), group, rows, tokens.device.index or 0, _stream_for(tokens))
    _raise_lib("stop_check", err)


@torch.library.custom_op("qqq_amd::stop_check", mutates_args=("n_seen", "n_trim", "stop_hit", "ids", "pos", "slots", "start", "remaining"))
def _stop_check_op(tokens: torch.Tensor, base: torch.Tensor, first: Optional[torch.Tensor], n_out: torch.Tensor, stop_ids: torch.Tensor,
                   stop_len: torch.Tensor, end_ids: torch.Tensor, eos: Optional[torch.Tensor], min_new: torch.Tensor, n_seen: torch.Tensor,
                   n_trim: torch.Tensor, stop_hit: torch.Tensor, ids: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor,
                   start: Optional[torch.Tensor], remaining: torch.Tensor) -> None:
    _stop_check_impl(tokens, base, first, n_out, stop_ids, stop_len, end_ids, eos, min_new, n_seen, n_trim, stop_hit, ids, pos, slots, start,
                     remaining)


@_stop_check_op.register_fake
def _(tokens, base, first, n_out, stop_ids, stop_len, end_ids, eos, min_new, n_seen, n_trim, stop_hit, ids, pos, slots, start, remaining):
    _stop_check_check(tokens, base, first, n_out, stop_ids, stop_len, end_ids, eos, min_new, n_seen, n_trim, stop_hit, ids, pos, slots,
                      start, remaining)


def stop_check(tokens: torch.Tensor, base: torch.Tensor, first: Optional[torch.Tensor], n_out: torch.Tensor, stop_ids: torch.Tensor,
               stop_len: torch.Tensor, min_new: torch.Tensor, n_seen: torch.Tensor, n_trim: torch.Tensor, stop_hit: torch.Tensor,
               ids: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor, remaining: torch.Tensor, start: Optional[torch.Tensor] = None,
               end_ids: Optional[torch.Tensor] = None, eos: Optional[torch.Tensor] = None) -> None:
    """A decode loop's stop epilogue, behind sample_advance / spec_advance (and topk_logprobs_step): a row whose completion has run into a
    stop sequence or a stop token id retires, in one launch.  Returns nothing; n_seen, n_trim, stop_hit, ids, pos, slots, start and
    remaining are updated in place.

    tokens, base, first   the completion of row r has n_out[r] + 1 tokens; token i is first[r] if base[r] + i < 0, else
                 tokens[r, base[r] + i].  tokens int32 or int64 [rows, stride], base int32 [rows], first int32 [rows] or None.  DecodeLoop
                 passes `out` with base -1 and the prefill's token, SpecDecodeLoop `hist` with base = the prompt's length
    stop_ids, stop_len   int32 [n_stop <= 32, stop_stride <= 32] and int32 [n_stop]: the stop sequences and their lengths, 0 = unused
    end_ids      int32 [at most 32] or None: the stop token ids, an entry < 0 unused
    eos          int32 [rows] or None: the rows' eos ids (-1: none), the array the sampler's step took
    min_new      int32 [rows]: no stop sequence is tested at a length below it;  n_seen  int32 [rows]: the length checked so far
    n_trim, stop_hit   int32 [rows]: on a match, the tokens the caller drops from the completion's end and the entry that matched
    ids, pos, slots   int64 [rows] or [rows, G <= 16];  start  int64 [rows] or None;  remaining  int32 [rows]: the row state to retire
    Every length n_seen[r] < e <= n_out[r] + 1 is tested in order; the first that ends in the row's eos or in an end id (the token
    stays; they go before a sequence that ends in the same token) or, from min_new[r] on, in a stop sequence (the completion is cut in
    front of it) retires the row: ids 0, pos / slots / start -1, remaining 0.
    Then n_seen[r] = n_out[r] + 1.  A row with nothing new writes nothing.  The exact semantics are stated in
    include/qqq_amd_stop.h.  Nothing is read on the host and the launch size depends on the shapes alone, so a decode
    step with this call in it replays from a captured graph."""
    if not isinstance(tokens, torch.Tensor) or not isinstance(ids, torch.Tensor) or tokens.dim() != 2:
        raise RuntimeError("stop_check: tokens must be an int32 or int64 [rows, stride] tensor and ids an int64 [rows] or [rows, group] tensor")
    if end_ids is None:
        end_ids = n_out.new_empty((0,), dtype=torch.int32)
    args = (tokens, base, first, n_out, stop_ids, stop_len, end_ids, eos, min_new, n_seen, n_trim, stop_hit, ids, pos, slots, start, remaining)
    if _compiling(*(t for t in args if t is not None)):
        return _stop_check_op(*args)
    return _stop_check_impl(*args)


# ---- beam search (include/qqq_amd_beam.h): the step behind a pass's logits, and the block copies of a cache reorder

class BeamStep(NamedTuple):
    """What beam_step returns.  cand_* and next_parent are views of `packed` (int32, the f32 arrays bit for bit), so that one copy of
    `packed` brings everything the host's bookkeeping reads; unpack_beam_step(packed.cpu(), prompts, num_beams) cuts it up again."""
    cand_score: torch.Tensor
    cand_logprob: torch.Tensor
    cand_parent: torch.Tensor
    cand_token: torch.Tensor
    next_ids: torch.Tensor
    next_parent: torch.Tensor
    next_cum: torch.Tensor
    next_live: torch.Tensor
    packed: torch.Tensor


def unpack_beam_step(packed: torch.Tensor, prompts: int, num_beams: int):
    """beam_step's packed int32 [prompts * 9 * num_beams] -> (cand_score f32, cand_logprob f32, cand_parent int32, cand_token int32, each
    [prompts, 2 * num_beams], next_parent int32 [prompts * num_beams]), as views."""
    c = prompts * 2 * num_beams
    return (packed[:c].view(torch.float32).view(prompts, -1), packed[c:2 * c].view(torch.float32).view(prompts, -1),
            packed[2 * c:3 * c].view(prompts, -1), packed[3 * c:4 * c].view(prompts, -1), packed[4 * c:])


def beam_step_workspace(rows: int, num_beams: int, device) -> torch.Tensor:
    """A workspace for beam_step over `rows` rows: int32 [4 * rows * num_beams] (the rows' candidates between the op's two launches).
    One workspace serves call after call on one stream."""
    return torch.empty((4 * rows * num_beams,), dtype=torch.int32, device=device)


def _beam_step_check(logits, cum, live, num_beams, workspace):
    # dtypes and shapes: needs no device, shared by the launch and the fake implementation -> (rows, vocab, prompts)
    op = "beam_step"
    if logits.dtype != torch.float16 or logits.dim() != 2:
        raise RuntimeError(f"{op}: logits must be fp16 [prompts * num_beams, vocab]")
    rows, vocab = logits.shape
    if num_beams < 1 or num_beams > 16:
        raise ValueError(f"{op}: num_beams={num_beams} outside [1, 16]")
    if rows % num_beams or rows > 65535:
        raise RuntimeError(f"{op}: logits hold {rows} rows: no multiple of num_beams={num_beams}, or more than 65535")
    if vocab < 2 * num_beams or vocab > 262144:
        raise RuntimeError(f"{op}: vocab={vocab} outside [2 * num_beams = {2 * num_beams}, 262144]")
    if cum.dtype != torch.float32 or cum.dim() != 1 or cum.shape[0] != rows:
        raise RuntimeError(f"{op}: cum must be f32 [{rows}], one entry per row, not {_dt(cum.dtype)} {tuple(cum.shape)}")
    if live.dtype != torch.int32 or live.dim() != 1 or live.shape[0] != rows:
        raise RuntimeError(f"{op}: live must be int32 [{rows}], one entry per row, not {_dt(live.dtype)} {tuple(live.shape)}")
    need = 4 * rows * num_beams
    if workspace.dtype != torch.int32 or workspace.dim() != 1 or workspace.shape[0] < need:
        raise RuntimeError(f"{op}: workspace must be int32 [at least {need}] (beam_step_workspace), not {_dt(workspace.dtype)} "
                           f"{tuple(workspace.shape)}")
    return rows, vocab, rows // num_beams


def _beam_step_outputs(like, rows, prompts, num_beams):
    return (like.new_empty((prompts * 9 * num_beams,), dtype=torch.int32), like.new_empty((rows,), dtype=torch.int64),
            like.new_empty((rows,), dtype=torch.float32), like.new_empty((rows,), dtype=torch.int32))


def _beam_step_impl(logits, cum, live, num_beams, eos, workspace):
    ts = (logits, cum, live, workspace)
    _same_gpu("beam_step", ts)
    rows, vocab, prompts = _beam_step_check(logits, cum, live, num_beams, workspace)
    packed, next_ids, next_cum, next_live = _beam_step_outputs(logits, rows, prompts, num_beams)
    if rows == 0:
        return packed, next_ids, next_cum, next_live
    _in_place_check("beam_step", (("cum", cum), ("live", live), ("workspace", workspace)))
    logits = _logits_rows(logits, vocab)
    c = prompts * 2 * num_beams  # the packed layout: cand_score, cand_logprob, cand_parent, cand_token [prompts, 2B], next_parent [rows]
    at = lambda i: packed.data_ptr() + 4 * c * i  # noqa: E731
    err = _lib.lib().qqq_beam_step(_ptr(logits), logits.stride(0), _ptr(cum), _ptr(live), at(0), at(1), at(2), at(3), _ptr(next_ids), at(4),
                                   _ptr(next_cum), _ptr(next_live), _ptr(workspace), 4 * workspace.shape[0], num_beams, eos, rows, vocab,
                                   logits.device.index or 0, _stream_for(logits))
    _raise_lib("beam_step", err)
    return packed, next_ids, next_cum, next_live


@torch.library.custom_op("qqq_amd::beam_step", mutates_args=("workspace",))
def _beam_step_op(logits: torch.Tensor, cum: torch.Tensor, live: torch.Tensor, num_beams: int, eos: int,
                  workspace: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return _beam_step_impl(logits, cum, live, num_beams, eos, workspace)


@_beam_step_op.register_fake
def _(logits, cum, live, num_beams, eos, workspace):
    rows, _, prompts = _beam_step_check(logits, cum, live, num_beams, workspace)
    return _beam_step_outputs(logits, rows, prompts, num_beams)


def beam_step(logits: torch.Tensor, cum: torch.Tensor, live: torch.Tensor, num_beams: int, eos: Optional[int] = None,
              workspace: Optional[torch.Tensor] = None) -> BeamStep:
    """One step of beam search behind a pass's fp16 logits [P * B, vocab] (row p * B + b: beam b of prompt p): a launch over the rows and one
    that merges them -> BeamStep.

    cum          f32 [P * B]: the beams' summed log-probabilities;  live  int32 [P * B]: a row with 0 contributes nothing
    num_beams    B, 1 ... 16;  eos  the id that ends a hypothesis, None or -1 for none
    workspace    int32, from beam_step_workspace(rows, B, device); None: a new one per call
    Every live row yields topk_logprobs' first 2B tokens; a candidate (b, i) has score = cum + that op's log-probability, one f32 addition;
    a prompt's candidates are ordered by score descending (NaN and -inf last), then b, then i, and the first 2B are cand_score,
    cand_logprob, cand_parent, cand_token [P, 2B].  The first B of them whose token is not eos become the next beams: next_ids int64 (the
    next pass's input, on the device), next_parent int32, next_cum f32, next_live int32, each [P * B].  A prompt without a live row writes
    parent = token = -1, score -inf and stays dead.  The exact semantics are stated in include/qqq_amd_beam.h.  Nothing is read on
    the host and the launch size depends on the shapes alone, so a captured graph replays with other contents.  A view whose rows are
    `vocab` columns of a wider, 16-byte aligned fp16 matrix (row stride a multiple of 8) is read in place."""
    if not isinstance(logits, torch.Tensor) or not isinstance(cum, torch.Tensor) or not isinstance(live, torch.Tensor) or logits.dim() != 2:
        raise RuntimeError("beam_step: logits must be an fp16 [prompts * num_beams, vocab] tensor, cum an f32 and live an int32 [rows] tensor")
    num_beams, eos = int(num_beams), -1 if eos is None else int(eos)
    if workspace is None:
        workspace = beam_step_workspace(logits.shape[0], max(num_beams, 1), logits.device)
    args = (logits, cum, live, num_beams, eos, workspace)
    packed, next_ids, next_cum, next_live = _beam_step_op(*args) if _compiling(logits, cum, live, workspace) else _beam_step_impl(*args)
    score, lp, parent, token, next_parent = unpack_beam_step(packed, logits.shape[0] // num_beams, num_beams)
    return BeamStep(score, lp, parent, token, next_ids, next_parent, next_cum, next_live, packed)


def _copy_blocks_check(pools, src, dst, block_bytes, num_blocks):
    # dtypes and shapes -> n
    op = "copy_blocks"
    if pools.dtype != torch.int64 or pools.dim() != 1 or not 1 <= pools.shape[0] <= 65535:
        raise RuntimeError(f"{op}: pools must be int64 [1 ... 65535 base addresses], not {_dt(pools.dtype)} {tuple(pools.shape)}")
    for name, t in (("src", src), ("dst", dst)):
        if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != src.shape[0]:
            raise RuntimeError(f"{op}: {name} must be int32 [n], one entry per copy, not {_dt(t.dtype)} {tuple(t.shape)}")
    if block_bytes < 16 or block_bytes % 16 or num_blocks < 1:
        raise ValueError(f"{op}: block_bytes={block_bytes} must be a positive multiple of 16 and num_blocks={num_blocks} at least 1")
    return src.shape[0]


def _copy_blocks_impl(pools, src, dst, block_bytes, num_blocks):
    ts = (pools, src, dst)
    _same_gpu("copy_blocks", ts)
    n = _copy_blocks_check(pools, src, dst, block_bytes, num_blocks)
    if n == 0:
        return
    _in_place_check("copy_blocks", (("pools", pools), ("src", src), ("dst", dst)))
    err = _lib.lib().qqq_copy_blocks(_ptr(pools), pools.shape[0], _ptr(src), _ptr(dst), n, block_bytes, num_blocks, pools.device.index or 0,
                                     _stream_for(pools))
    _raise_lib("copy_blocks", err)


@torch.library.custom_op("qqq_amd::copy_blocks", mutates_args=())
def _copy_blocks_op(pools: torch.Tensor, src: torch.Tensor, dst: torch.Tensor, block_bytes: int, num_blocks: int) -> None:
    _copy_blocks_impl(pools, src, dst, block_bytes, num_blocks)


@_copy_blocks_op.register_fake
def _(pools, src, dst, block_bytes, num_blocks):
    _copy_blocks_check(pools, src, dst, block_bytes, num_blocks)


def copy_blocks(pools: torch.Tensor, src: torch.Tensor, dst: torch.Tensor, block_bytes: int, num_blocks: int) -> None:
    """Copy block src[j] to block dst[j] in every pool of a table, in one launch (PagedKVCache.reorder's partial-block copies).

    pools        int64 [n_pools] on the device: the pools' base addresses (tensor.data_ptr()), every pool [num_blocks] blocks of
                 block_bytes bytes (a multiple of 16), 16-byte aligned.  The caller keeps the pools alive; the op sees addresses only.
    src, dst     int32 [n] on the device; the dst entries are distinct and none equals a src entry, one src may feed several dst; an id
                 outside [0, num_blocks) copies nothing.  n = 0 is a no-op.
    Nothing is read on the host.  The exact semantics are stated in include/qqq_amd_beam.h."""
    if not all(isinstance(t, torch.Tensor) for t in (pools, src, dst)):
        raise RuntimeError("copy_blocks: pools must be an int64 [n_pools] tensor, src and dst int32 [n] tensors")
    args = (pools, src, dst, int(block_bytes), int(num_blocks))
    if _compiling(pools, src, dst):
        return _copy_blocks_op(*args)
    return _copy_blocks_impl(*args)


# ---- guided decoding (include/qqq_amd_guided.h): the mask in front of a sampler, the advance behind a loop's step

def _fsm_tables_check(op, fsm_tensors):
    # the automaton's four CSR arrays -> (n_states, n_edges)
    if not isinstance(fsm_tensors, (tuple, list)) or len(fsm_tensors) != 4 or not all(isinstance(t, torch.Tensor) for t in fsm_tensors):
        raise RuntimeError(f"{op}: fsm_tensors must be the four tensors (offsets, tokens, next, accept) of TokenFSM.tensors()")
    offsets, tokens, nxt, accept = fsm_tensors
    for name, t in (("offsets", offsets), ("tokens", tokens), ("next", nxt), ("accept", accept)):
        if t.dtype != torch.int32 or t.dim() != 1:
            raise RuntimeError(f"{op}: {name} must be int32 and one-dimensional, not {_dt(t.dtype)} {tuple(t.shape)}")
    if accept.shape[0] < 1 or offsets.shape[0] != accept.shape[0] + 1:
        raise RuntimeError(f"{op}: accept must hold S >= 1 states and offsets S + 1 entries, not {tuple(accept.shape)} and {tuple(offsets.shape)}")
    if nxt.shape[0] != tokens.shape[0]:
        raise RuntimeError(f"{op}: next must hold one entry per edge like tokens {tuple(tokens.shape)}, not {tuple(nxt.shape)}")
    return accept.shape[0], tokens.shape[0]


def _fsm_mask_check(logits, state, offsets, tokens, nxt, accept, eos, remaining):
    # dtypes, shapes and strides -> (rows, vocab, n_states, n_edges)
    op = "fsm_mask"
    if logits.dtype != torch.float16 or logits.dim() != 2:
        raise RuntimeError(f"{op}: logits must be fp16 [rows, vocab]")
    rows, vocab = logits.shape
    _rows_i32_check(op, rows, [("state", state)] + ([("eos", eos)] if eos is not None else []) +
                    ([("remaining", remaining)] if remaining is not None else []))
    n_states, n_edges = _fsm_tables_check(op, (offsets, tokens, nxt, accept))
    if vocab < 1 or vocab > 262144 or rows > 65535:
        raise RuntimeError(f"{op}: logits {tuple(logits.shape)} outside 1 <= vocab <= 262144, rows <= 65535")
    if rows and (logits.stride(1) != 1 or logits.stride(0) < vocab):
        raise RuntimeError(f"{op}: logits must have unit column stride and a row stride >= vocab (they are rewritten in place, never "
                           f"copied), not strides {tuple(logits.stride())}")
    return rows, vocab, n_states, n_edges


def _fsm_mask_impl(logits, state, offsets, tokens, nxt, accept, eos, remaining):
    names = ("logits", "state", "offsets", "tokens", "next", "accept", "eos", "remaining")
    given = [(n, t) for n, t in zip(names, (logits, state, offsets, tokens, nxt, accept, eos, remaining)) if t is not None]
    _same_gpu("fsm_mask", [t for _, t in given])
    rows, vocab, n_states, n_edges = _fsm_mask_check(logits, state, offsets, tokens, nxt, accept, eos, remaining)
    if rows == 0:
        return
    _in_place_check("fsm_mask", given[1:])
    err = _lib.lib().qqq_fsm_mask(_ptr(logits), logits.stride(0), _ptr(state), _ptr(eos), _ptr(remaining), _ptr(offsets), _ptr(tokens),
                                  _ptr(accept), n_states, n_edges, rows, vocab, logits.device.index or 0, _stream_for(logits))
    _raise_lib("fsm_mask", err)


@torch.library.custom_op("qqq_amd::fsm_mask", mutates_args=("logits",))
def _fsm_mask_op(logits: torch.Tensor, state: torch.Tensor, offsets: torch.Tensor, tokens: torch.Tensor, nxt: torch.Tensor,
                 accept: torch.Tensor, eos: Optional[torch.Tensor], remaining: Optional[torch.Tensor]) -> None:
    _fsm_mask_impl(logits, state, offsets, tokens, nxt, accept, eos, remaining)


@_fsm_mask_op.register_fake
def _(logits, state, offsets, tokens, nxt, accept, eos, remaining):
    _fsm_mask_check(logits, state, offsets, tokens, nxt, accept, eos, remaining)


def fsm_mask(logits: torch.Tensor, state: torch.Tensor, fsm_tensors, eos: Optional[torch.Tensor] = None,
             remaining: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Guided decoding's mask on fp16 logits [rows, vocab], in place and in one launch, in front of sample_tokens or sample_advance (behind
    penalize_logits and ban_tokens) -> `logits`.

    state        int32 [rows]: the rows' states in the automaton; a row whose state is outside [0, S) -- -1: no automaton -- is untouched
    fsm_tensors  (offsets int32 [S + 1], tokens int32 [E], next int32 [E], accept int32 [S]): TokenFSM.tensors(device), or a loop's buffers
    eos          int32 [rows] or None: the rows' eos ids (-1: none), allowed in an accepting state
    remaining    int32 [rows] or None: a decode loop's budgets; a row with 0 is idle and untouched
    Every column of [0, vocab) that is neither a token of the row's state nor its allowed eos becomes -inf; an allowed column keeps its
    bits, and the logits are never read.  The exact semantics are stated in include/qqq_amd_guided.h.  Nothing is read on the
    host and the launch size depends on the shapes alone, so a step with this call in it replays from a captured graph.  The logits are
    never copied: unit column stride and a row stride >= vocab, or it raises."""
    if not isinstance(logits, torch.Tensor) or not isinstance(state, torch.Tensor) or logits.dim() != 2 or state.dim() != 1:
        raise RuntimeError("fsm_mask: logits must be an fp16 [rows, vocab] tensor and state an int32 [rows] tensor")
    _fsm_tables_check("fsm_mask", fsm_tensors)
    args = (logits, state, *fsm_tensors, eos, remaining)
    if _compiling(*(t for t in args if t is not None)):
        _fsm_mask_op(*args)
    else:
        _fsm_mask_impl(*args)
    return logits


def _fsm_advance_check(out, n_out, n_fsm, state, offsets, tokens, nxt, accept, ids, pos, slots, remaining, eos):
    # dtypes and shapes -> (rows, n_states, n_edges)
    op = "fsm_advance"
    if out.dtype != torch.int64 or out.dim() != 2 or out.shape[1] < 1:
        raise RuntimeError(f"{op}: out must be int64 [rows, out_stride >= 1], not {_dt(out.dtype)} {tuple(out.shape)}")
    rows = out.shape[0]
    _rows_i32_check(op, rows, [("n_out", n_out), ("n_fsm", n_fsm), ("state", state), ("remaining", remaining)] +
                    ([("eos", eos)] if eos is not None else []))
    for name, t in (("ids", ids), ("pos", pos), ("slots", slots)):
        if t.dtype != torch.int64 or t.dim() != 1 or t.shape[0] != rows:
            raise RuntimeError(f"{op}: {name} must be int64 [{rows}], not {_dt(t.dtype)} {tuple(t.shape)}")
    n_states, n_edges = _fsm_tables_check(op, (offsets, tokens, nxt, accept))
    if rows > 65535:
        raise RuntimeError(f"{op}: rows={rows} exceeds 65535")
    return rows, n_states, n_edges


def _fsm_advance_impl(out, n_out, n_fsm, state, offsets, tokens, nxt, accept, ids, pos, slots, remaining, eos):
    names = ("out", "n_out", "n_fsm", "state", "offsets", "tokens", "next", "accept", "ids", "pos", "slots", "remaining", "eos")
    args = (out, n_out, n_fsm, state, offsets, tokens, nxt, accept, ids, pos, slots, remaining, eos)
    given = [(n, t) for n, t in zip(names, args) if t is not None]
    _same_gpu("fsm_advance", [t for _, t in given])
    rows, n_states, n_edges = _fsm_advance_check(*args)
    if rows == 0:
        return
    _in_place_check("fsm_advance", given)
    err = _lib.lib().qqq_fsm_advance(_ptr(out), out.shape[1], _ptr(n_out), _ptr(n_fsm), _ptr(state), _ptr(eos), _ptr(offsets), _ptr(tokens),
                                     _ptr(nxt), _ptr(accept), n_states, n_edges, _ptr(ids), _ptr(pos), _ptr(slots), _ptr(remaining), rows,
                                     out.device.index or 0, _stream_for(out))
    _raise_lib("fsm_advance", err)


@torch.library.custom_op("qqq_amd::fsm_advance", mutates_args=("n_fsm", "state", "ids", "pos", "slots", "remaining"))
def _fsm_advance_op(out: torch.Tensor, n_out: torch.Tensor, n_fsm: torch.Tensor, state: torch.Tensor, offsets: torch.Tensor,
                    tokens: torch.Tensor, nxt: torch.Tensor, accept: torch.Tensor, ids: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor,
                    remaining: torch.Tensor, eos: Optional[torch.Tensor]) -> None:
    _fsm_advance_impl(out, n_out, n_fsm, state, offsets, tokens, nxt, accept, ids, pos, slots, remaining, eos)


@_fsm_advance_op.register_fake
def _(out, n_out, n_fsm, state, offsets, tokens, nxt, accept, ids, pos, slots, remaining, eos):
    _fsm_advance_check(out, n_out, n_fsm, state, offsets, tokens, nxt, accept, ids, pos, slots, remaining, eos)


def fsm_advance(out: torch.Tensor, n_out: torch.Tensor, n_fsm: torch.Tensor, state: torch.Tensor, fsm_tensors, ids: torch.Tensor,
                pos: torch.Tensor, slots: torch.Tensor, remaining: torch.Tensor, eos: Optional[torch.Tensor] = None) -> None:
    """Guided decoding's epilogue of a decode loop's step, behind sample_advance (and stop_check): every row's state moves on over the
    tokens it emitted since it was last advanced, in one launch.  Returns nothing; n_fsm, state, ids, pos, slots and remaining are
    updated in place.

    out, n_out   int64 [rows, out_stride] and int32 [rows]: the rows' emitted tokens and their counts (sample_advance's)
    n_fsm        int32 [rows]: the count up to which a row's state has been advanced;  state  int32 [rows]
    fsm_tensors  (offsets, tokens, next, accept) as for fsm_mask
    ids, pos, slots   int64 [rows];  remaining  int32 [rows]: the row state to retire;  eos  int32 [rows] or None
    A token with an edge moves the state to the edge's target, and a terminal target (no edges) retires the row: ids 0, pos / slots -1,
    remaining 0.  The row's eos without an edge in an accepting state leaves the state (the sampler retired the row).  Any other token
    sets the state to -2 and retires the row.  A state outside [0, S) stays.  Then n_fsm[r] = n_out[r]; a row with nothing new writes
    nothing.  The exact semantics are stated in include/qqq_amd_guided.h.  Nothing is read on the host and the launch size
    depends on the shapes alone, so a decode step with this call in it replays from a captured graph."""
    if not isinstance(out, torch.Tensor) or not isinstance(state, torch.Tensor) or out.dim() != 2:
        raise RuntimeError("fsm_advance: out must be an int64 [rows, out_stride] tensor and state an int32 [rows] tensor")
    _fsm_tables_check("fsm_advance", fsm_tensors)
    args = (out, n_out, n_fsm, state, *fsm_tensors, ids, pos, slots, remaining, eos)
    if _compiling(*(t for t in args if t is not None)):
        return _fsm_advance_op(*args)
    return _fsm_advance_impl(*args)


# ---- batched LoRA (include/qqq_amd_lora.h): low-rank fp16 adapters beside the W4A8 GEMM, every token's adapter on the device

def _lora_add_check(y, xq, s1, A, B, scale, slot, part_cols):
    # dtypes, shapes and strides -> (T, N, K, R, S, P); R's list, the offsets' rules and the alignment are the library's to refuse
    op = "lora_add"
    for name, t, dt in (("y", y, torch.float16), ("xq", xq, torch.int8), ("s1", s1, torch.float32), ("A", A, torch.float16),
                        ("B", B, torch.float16), ("scale", scale, torch.float32), ("slot", slot, torch.int32)):
        if t.dtype != dt:
            raise RuntimeError(f"{op}: {name} must be {_dt(dt)}, not {_dt(t.dtype)}")
    if y.dim() != 2 or xq.dim() != 2 or xq.shape[0] != y.shape[0]:
        raise RuntimeError(f"{op}: y must be fp16 [T, N] and xq int8 [T, K], not {tuple(y.shape)} and {tuple(xq.shape)}")
    (T, N), K = y.shape, xq.shape[1]
    if s1.numel() != T or s1.dim() not in (1, 2) or slot.dim() != 1 or slot.shape[0] != T:
        raise RuntimeError(f"{op}: s1 must be f32 [{T}] or [{T}, 1] and slot int32 [{T}], not {tuple(s1.shape)} and {tuple(slot.shape)}")
    P = len(part_cols) - 1
    if A.dim() != 3 or B.dim() != 3 or scale.dim() != 1 or P < 1:
        raise RuntimeError(f"{op}: A must be fp16 [S, P * R, K], B fp16 [S, N, R], scale f32 [S] and part_cols P + 1 >= 2 offsets")
    S, R = B.shape[0], B.shape[2]
    if A.shape != (S, P * R, K) or B.shape[1] != N or scale.shape[0] != S or S < 1:
        raise RuntimeError(f"{op}: with y {tuple(y.shape)}, xq {tuple(xq.shape)} and {P} part(s), A must be [S, {P} * R, {K}], B [S, {N}, R] and "
                           f"scale [S], not {tuple(A.shape)}, {tuple(B.shape)} and {tuple(scale.shape)}")
    if T and (y.stride(1) != 1 or y.stride(0) < N):
        raise RuntimeError(f"{op}: y must have unit column stride and a row stride >= N (it is updated in place, never copied), not strides "
                           f"{tuple(y.stride())}")
    if A.stride()[1:] != (K, 1) or B.stride()[1:] != (R, 1) or (S > 1 and (A.stride(0) < P * R * K or B.stride(0) < N * R)):
        raise RuntimeError(f"{op}: A and B must have contiguous rows and columns (only the slot stride is free), not strides "
                           f"{tuple(A.stride())} and {tuple(B.stride())}")
    return T, N, K, R, S, P


def _lora_add_impl(y, xq, s1, A, B, scale, slot, part_cols):
    _same_gpu("lora_add", (y, xq, s1, A, B, scale, slot))
    T, N, K, R, S, P = _lora_add_check(y, xq, s1, A, B, scale, slot, part_cols)
    if T == 0:
        return
    _in_place_check("lora_add", (("xq", xq), ("s1", s1), ("scale", scale), ("slot", slot)))
    cols = (ctypes.c_int * (P + 1))(*part_cols)
    err = _lib.lib().qqq_lora_add(_ptr(y), y.stride(0), _ptr(xq), _ptr(s1), _ptr(A), max(A.stride(0), P * R * K), _ptr(B),
                                  max(B.stride(0), N * R), _ptr(scale), _ptr(slot), cols, P, T, N, K, R, S, y.device.index or 0,
                                  _stream_for(y))
    _raise_lib("lora_add", err)


@torch.library.custom_op("qqq_amd::lora_add", mutates_args=("y",))
def _lora_add_op(y: torch.Tensor, xq: torch.Tensor, s1: torch.Tensor, A: torch.Tensor, B: torch.Tensor, scale: torch.Tensor,
                 slot: torch.Tensor, part_cols: Sequence[int]) -> None:
    _lora_add_impl(y, xq, s1, A, B, scale, slot, part_cols)


@_lora_add_op.register_fake
def _(y, xq, s1, A, B, scale, slot, part_cols):
    _lora_add_check(y, xq, s1, A, B, scale, slot, part_cols)


def lora_add(y: torch.Tensor, xq: torch.Tensor, s1: torch.Tensor, A: torch.Tensor, B: torch.Tensor, scale: torch.Tensor, slot: torch.Tensor,
             part_cols=None) -> torch.Tensor:
    """Batched LoRA beside the W4A8 GEMM, in place and in one launch -> `y`: every row adds its own adapter's low-rank product.

    y            fp16 [T, N]: the GEMM's output, bias included; unit column stride, an even row stride >= N, never copied
    xq, s1       int8 [T, K] and f32 [T] or [T, 1]: the quantised activation the GEMM consumed (dynamic_quant, rmsnorm_quant, ...)
    A, B, scale  fp16 [S, P * R, K], fp16 [S, N, R], f32 [S]: S adapter slots of rank R in {8, 16, 32, 64}; A and B may be views with
                 their own slot stride (rows and columns contiguous)
    slot         int32 [T] on the device: the row's slot; -1 -- or anything outside [0, S) -- leaves the row's bits alone
    part_cols    P + 1 column offsets (ints; a list, tuple or CPU tensor), ascending from 0 to N in multiples of 64: column n of part p
                 uses the rows p * R ... (p + 1) * R - 1 of A (q|k|v, gate|up).  None: one part, [0, N].
    For slot[t] = a >= 0:  y[t, n] <- fp16(float(y[t, n]) + scale[a] * sum_r B[a, n, r] * (s1[t] * sum_k A[a, p * R + r, k] * xq[t, k])),
    every product and sum in f32, one rounding.  A row's bits depend on that row and its slot's matrices alone, and a call with P parts
    gives the bits of P calls on the column slices.  The exact semantics are stated in include/qqq_amd_lora.h.  Nothing
    is read on the host and the launch size depends on the shapes alone, so a step with this call in it replays from a captured graph."""
    ts = (y, xq, s1, A, B, scale, slot)
    if not all(isinstance(t, torch.Tensor) for t in ts):
        raise RuntimeError("lora_add: y, xq, s1, A, B, scale and slot must be tensors")
    if part_cols is None:
        part_cols = (0, y.shape[-1])
    elif isinstance(part_cols, torch.Tensor):
        part_cols = part_cols.tolist()
    part_cols = tuple(int(c) for c in part_cols)
    if _compiling(*ts):
        _lora_add_op(*ts, part_cols)
    else:
        _lora_add_impl(*ts, part_cols)
    return y
