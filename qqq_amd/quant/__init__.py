"""qqq_amd.quant -- the GPTQ weight quantiser on the device: makes the (fake-quantised weight, scales) pair QuantLinear.pack takes, and
whole QQQ W4A8 checkpoints from fp16 ones, rotated first where asked.  A sub-package with a HIP library of its own
(libqqq_amd_quant.so, include/qqq_amd_quant.h and qqq_amd_rotate.h here): an offline tool, nothing of it is loaded by serving.

    ops.weight_scales, ops.gptq_block   the two HIP ops: a row's 4-bit scale (optionally the reference's shrink search) and the column
                                        sweep of one 128-column GPTQ block in one launch
    Hessian, gptq_quantize, GPTQResult  GPTQ of one linear (the reference's fasterquant in its order)
    group_scales, gptq_block_cols       (ops.*) the HIP ops of act-order with static groups: every group's scale in one launch, and the
                                        sweep with a scale per (row, column), looked up through the column's group
    gptq_quantize_ordered               fasterquant(actorder=True, static_groups=True): columns swept by falling diag(H), group scales
                                        found before the sweep, the result un-permuted -- an ordinary checkpoint; quantize_model(...,
                                        act_order=True, static_groups=True) is the reference's default recipe
    quantize_model                      the layer-wise flow over a Llama / Qwen2 state dict -> a packed QuantLlamaForCausalLM;
                                        rotation="hadamard" rotates the state dict first (the reference's default, with mse=True)
    ops.hadamard_rows, ops.check_signs  the third HIP op: the blocked Walsh-Hadamard transform of matrix rows, exact for fp16
    fuse_layer_norms, hadamard_signs,   rotation over state dicts (rotation.py): norms folded into the linears, the residual stream
    rotate_state_dict, rotate_model     turned by a randomised Hadamard (or any orthogonal) matrix, the per-head Hadamard on v / o

Out of scope: smoothing, Hadamard sizes that are no power of two, act-order with moving (non-static) groups, asymmetric modes, other bit
widths and group sizes."""
from . import ops
from .gptq import BlockTrace, GPTQResult, Hessian, gptq_quantize, gptq_quantize_ordered, round_to_nearest
from .model import FloatDecoderLayer, quantize_model
from .ops import gptq_block_cols, group_scales
from .rotation import fuse_layer_norms, hadamard_matrix, hadamard_signs, random_orthogonal, rotate_model, rotate_state_dict

__all__ = ["ops", "Hessian", "gptq_quantize", "gptq_quantize_ordered", "group_scales", "gptq_block_cols", "round_to_nearest", "GPTQResult",
           "BlockTrace", "FloatDecoderLayer", "quantize_model",
           "fuse_layer_norms", "hadamard_signs", "hadamard_matrix", "random_orthogonal", "rotate_state_dict", "rotate_model"]
