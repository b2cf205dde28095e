"""qqq_amd.quant -- the GPTQ weight quantiser on the device: makes the (fake-quantised weight, scales) pair QuantLinear.pack takes, and
whole QQQ W4A8 checkpoints from fp16 ones, rotated first where asked.  A sub-package with a HIP library of its own
(libqqq_amd_quant.so, the headers of include/, include_ext/ and include_ops/ here): an offline tool, nothing of it is loaded by serving.

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
    ops.hadamard_rows_k, ops.check_table  the HIP op for hidden sizes K * 2^p: the Sylvester stages of every sub-block and the K x K
                                        Hadamard table that mixes them, one launch; the table is an argument
    hadamard_table, hadamard_factor,    our tables for K = 12, 20, 28, 40 by construction, the (K, m) the reference picks for a size,
    hadamard_matrix_k                   and the dense Q of mode="hadamard_k" (rotate_model, quantize_model(rotation="hadamard_k"))

    ops.fake_quant_rows                 the HIP op of smoothing: a column-scaled fp16 operand fake-quantised per row or per (row, 128
                                        columns) in one launch, the bits of the reference's fourteen-launch torch composition
    migration_scale, smooth_scales,     smoothing over state dicts (smooth.py): the reference's os+ / awq / sq searches of a module's
    apply_smooth, smooth_model          migration scale, the layer-wise flow that makes its scale_list, and the fold into the weights
                                        (quantize_model(..., smooth="os+"), after rotation and before GPTQ)

Out of scope: token-wise clipping after smoothing, Hadamard tables of other orders (pass one as table=), a head_dim that is no power of two, act-order with moving (non-static) groups, asymmetric modes, other bit
widths and group sizes."""
from . import ops
from .gptq import BlockTrace, GPTQResult, Hessian, gptq_quantize, gptq_quantize_ordered, round_to_nearest
from .model import FloatDecoderLayer, quantize_model
from .ops import gptq_block_cols, group_scales
from .ops import check_table, hadamard_rows_k
from .ops import fake_quant_rows
from .smooth import apply_smooth, migration_scale, smooth_model, smooth_scales
from .rotation import (fuse_layer_norms, hadamard_factor, hadamard_matrix, hadamard_matrix_k, hadamard_signs, hadamard_table,
                       random_orthogonal, rotate_model, rotate_state_dict)

__all__ = ["ops", "Hessian", "gptq_quantize", "gptq_quantize_ordered", "group_scales", "gptq_block_cols", "round_to_nearest", "GPTQResult",
           "BlockTrace", "FloatDecoderLayer", "quantize_model",
           "fuse_layer_norms", "hadamard_signs", "hadamard_matrix", "random_orthogonal", "rotate_state_dict", "rotate_model",
           "hadamard_rows_k", "check_table", "hadamard_table", "hadamard_factor", "hadamard_matrix_k",
           "fake_quant_rows", "migration_scale", "smooth_scales", "apply_smooth", "smooth_model"]
