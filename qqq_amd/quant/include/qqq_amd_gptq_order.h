/*
 * qqq_amd_gptq_order.h -- C-ABI of the two device ops GPTQ needs for act-order with static groups (libqqq_amd_quant.so, beside
 * qqq_amd_quant.h, whose four prototypes and ABI version stay as they are, and qqq_amd_rotate.h).  With act-order the columns are swept
 * by falling diag(H); with static groups every group's scale is found once, before the sweep, from the unswept weight.  A 128-column block
 * of the permuted order then holds columns of many groups, and the sweep needs a scale per (row, column).  The flow is
 * qqq_amd/quant/gptq.py, gptq_quantize_ordered.
 *
 * All matrices are f32, row-major with a row stride in elements, 4-byte aligned; the arithmetic is the grouped mode of qqq_amd_quant.h:
 *   codes 0 ... 15, zero 8     quantise(w, s) = s * (clamp(rint(w / s) + 8, 0, 15) - 8)
 *
 * qqq_gptq_group_scales   the scale of every group of 128 columns of every row, one launch:
 *   W           f32 [rows, cols], row stride ldw >= cols;  cols a multiple of 128, 128 <= cols <= 1048576;  rows >= 1
 *   scales_out  f32 [rows, cols / 128], row stride lds >= cols / 128
 *   scales_out[r, g] has the bits qqq_gptq_scales(W + 128 g, ldw, rows, 128, grouped = 1, mse, ...) writes for row r: (xmax + xmax) / 15
 *   of the group's max |w| (1 for an all-zero group), with mse != 0 the shrink search over 80 ranges of qqq_amd_quant.h, its sums in
 *   the same order.  An entry depends on its 128 values alone.  scales_out must not overlap W.
 *
 * qqq_gptq_block_cols     the column sweep of qqq_gptq_block in grouped arithmetic with the scale of step i looked up through the
 *   column's group: for i = 0 ... count - 1 and every row r
 *       s = scales[r, clamp(gidx[i], 0, groups - 1)]
 *       q = quantise(W1[r, i], s)
 *       e = (W1[r, i] - q) / Hinv1[i, i]
 *       W1[r, j] = W1[r, j] - (e * Hinv1[i, j])    for j = i ... count - 1: the product rounded, then subtracted
 *       Q1[r, i] = q;  Err1[r, i] = e
 *   W1, Hinv1, Q1, Err1   as qqq_gptq_block's: W1 is read and not written, only the upper triangle of Hinv1 is used
 *   scales  f32 [rows, groups], row stride lds >= groups, groups >= 1
 *   gidx    int32 [count] in DEVICE memory: read by the kernel, never on the host, so a captured launch replays with other contents.
 *           An index outside [0, groups) is clamped into the range inside the kernel: no content of gidx reads out of bounds.
 *   count in {64, 128}, rows >= 1, every matrix stride >= count.  A row's bits depend on that row, Hinv1, its row of scales and gidx
 *   alone: not on rows, nor on the row's place in the launch.  With every gidx[i] == g the bits are those of
 *   qqq_gptq_block(..., scale = scales[:, g], grouped = 1).  Q1 and Err1 must not overlap W1, Hinv1, scales or gidx.
 *
 * Conventions are those of qqq_amd_quant.h: work is only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state,
 * one launch per call whose size depends on the shapes alone.  Return codes QQQ_OK (0) / QQQ_ERR_ARG / QQQ_ERR_HIP with the values of
 * include/qqq_amd.h, and a message in qqq_quant_last_error() (thread-local) that begins with the entry's name; bad arguments are
 * rejected before any launch.
 */
#ifndef QQQ_AMD_GPTQ_ORDER_H_
#define QQQ_AMD_GPTQ_ORDER_H_

#ifdef __cplusplus
extern "C" {
#endif

int qqq_gptq_group_scales(const void* W, int ldw, int rows, int cols, int mse, void* scales_out, int lds, int dev, void* stream);

int qqq_gptq_block_cols(const void* W1, int ldw, const void* Hinv1, int ldh, const void* scales, int lds, int groups, const void* gidx,
                        int rows, int count, void* Q1, int ldq, void* Err1, int lde, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_GPTQ_ORDER_H_ */
