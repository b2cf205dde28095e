"""qqq_amd.quant -- the GPTQ weight quantiser on the device: makes the (fake-quantised weight, scales) pair QuantLinear.pack takes, and
whole QQQ W4A8 checkpoints from fp16 ones.  A sub-package with a HIP library of its own (libqqq_amd_quant.so, include/qqq_amd_quant.h
here): an offline tool, nothing of it is loaded by serving.

    ops.weight_scales, ops.gptq_block   the two HIP ops: a row's 4-bit scale (optionally the reference's shrink search) and the column
                                        sweep of one 128-column GPTQ block in one launch
    Hessian, gptq_quantize, GPTQResult  GPTQ of one linear (the reference's fasterquant in its order)
    quantize_model                      the layer-wise flow over a Llama / Qwen2 state dict -> a packed QuantLlamaForCausalLM

Out of scope: rotation and smoothing (pure weight algebra in front of this; `mse=True` is the reference's pairing for rotated models),
act-order, static groups, asymmetric modes, other bit widths and group sizes."""
from . import ops
from .gptq import BlockTrace, GPTQResult, Hessian, gptq_quantize, round_to_nearest
from .model import FloatDecoderLayer, quantize_model

__all__ = ["ops", "Hessian", "gptq_quantize", "round_to_nearest", "GPTQResult", "BlockTrace", "FloatDecoderLayer", "quantize_model"]
