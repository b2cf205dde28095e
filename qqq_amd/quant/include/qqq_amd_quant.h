/*
 * qqq_amd_quant.h -- C-ABI of the GPTQ weight quantiser (exported by libqqq_amd_quant.so, a library of its own beside libqqq_amd.so: the
 * quantiser is an offline tool and adds nothing to the serving library).  Two device ops; everything else of GPTQ (Hessian, Cholesky,
 * the trailing GEMM between blocks) is plain torch in qqq_amd/quant/gptq.py.
 *
 * All matrices are f32, row-major with a row stride in elements, 4-byte aligned.  Only the two symmetric 4-bit modes QuantLinear.pack
 * holds exist:
 *   per-channel (grouped = 0)   codes -7 ... 7            quantise(w, s) = s * clamp(rint(w / s), -7, 7)
 *   grouped     (grouped = 1)   codes 0 ... 15, zero 8    quantise(w, s) = s * (clamp(rint(w / s) + 8, 0, 15) - 8)
 * in IEEE f32: a correctly rounded divide, rint = round half to even, subnormals kept.
 *
 * qqq_gptq_scales   the scale of every row of W[:, 0:cols] (the reference's Quantizer.find_params(..., weight=True)):
 *   W          f32 [rows, cols], row stride ldw >= cols;   scale_out  f32 [rows]
 *   xmax = max |w| over the row, 1 for an all-zero row;  s = xmax / 7 (per-channel),  s = (xmax + xmax) / 15 (grouped)
 *   mse != 0: the shrink search.  Candidate i = 0 ... 79 has the range r_i = f32(1 - i / 100) * xmax, its scale s_i formed from r_i as s
 *   is from xmax, and the error sum |quantise(w, s_i) - w| ^ 2.4 over the row; the row takes the candidate of the least error, the
 *   earliest on a tie (strict <).  The sums are f32 in an order of the kernel's own: the choice is that of exact sums wherever the
 *   runner-up is more than a relative 1e-4 away.
 *   1 <= rows, 1 <= cols <= 1048576.  A row's result depends on that row alone.
 *
 * qqq_gptq_block    the column sweep of one GPTQ block: for i = 0 ... count - 1 and every row r, in this f32 arithmetic
 *       q = quantise(W1[r, i], scale[r])
 *       e = (W1[r, i] - q) / Hinv1[i, i]
 *       W1[r, j] = W1[r, j] - (e * Hinv1[i, j])    for j = i ... count - 1: the product rounded, then subtracted (no fused multiply-add)
 *       Q1[r, i] = q;  Err1[r, i] = e
 *   W1    f32 [rows, count], row stride ldw: read, not written (the reference never reads the swept block again)
 *   Hinv1 f32 [count, count], row stride ldh: the block on the diagonal of the upper Cholesky factor of the inverse Hessian; only its
 *         upper triangle is used
 *   scale f32 [rows];  Q1, Err1  f32 [rows, count], row strides ldq, lde
 *   count in {64, 128}, rows >= 1, every stride >= count.  A row's bits depend on that row, Hinv1 and its scale alone: not on rows, nor on
 *   the row's place in the launch.  Q1 and Err1 must not overlap W1, Hinv1 or scale.
 *
 * Conventions are those of include/qqq_amd.h: work is only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state,
 * one launch per call whose size depends on the shapes alone.  Return codes QQQ_OK (0) / QQQ_ERR_ARG / QQQ_ERR_HIP with the values of
 * qqq_amd.h, and a message in qqq_quant_last_error() (thread-local) that begins with the entry's name; bad arguments are rejected before
 * any launch.
 */
#ifndef QQQ_AMD_QUANT_H_
#define QQQ_AMD_QUANT_H_

#include <stddef.h>

#define QQQ_AMD_QUANT_ABI_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

int qqq_quant_abi_version(void);
const char* qqq_quant_last_error(void);

int qqq_gptq_scales(const void* W, int ldw, int rows, int cols, int grouped, int mse, void* scale_out, int dev, void* stream);

int qqq_gptq_block(const void* W1, int ldw, const void* Hinv1, int ldh, const void* scale, int rows, int count, int grouped, void* Q1,
                   int ldq, void* Err1, int lde, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_QUANT_H_ */
