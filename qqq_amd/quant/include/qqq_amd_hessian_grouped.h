/*
 * qqq_amd_hessian_grouped.h -- C-ABI of the grouped Hessian accumulation op of the quantiser's library (libqqq_amd_quant.so; beside
 * qqq_amd_hessian.h, whose prototype, like the ABI version of qqq_amd_quant.h, stays as it is).  One device op: the running Hessians of
 * ALL experts of a mixture-of-experts layer over one calibration batch, each over the rows routed to it, in one launch that follows the
 * routing where qqq_moe_route (include/qqq_amd_moe.h) left it -- on the device.
 *
 * qqq_hessian_update_grouped   for every expert e < E with c_e = offsets[e + 1] - offsets[e] > 0:
 *                                H_e[i][j] <- f32( f32(alpha[e] * H_e[i][j]) + f32(beta[e] * S_e[i][j]) )  for EVERY i, j < n,
 *                                S_e = sum over the positions offsets[e] <= p < offsets[e + 1], in that order, of x_p[i] * x_p[j],
 *                                x_p = X[order[p] / a_div]
 *   H        f32 [E, n, n]: expert stride lde >= n * ldh in ELEMENTS and a multiple of 4 (a size_t: E * lde passes 2^31), row stride
 *            ldh >= n and a multiple of 4; 16-byte aligned.  As qqq_hessian_update: the whole symmetric matrix is written, every entry
 *            from its own old value, bit-symmetric; nothing between the rows or between the matrices is touched.
 *            c_e == 0: H_e is neither read nor written.   alpha[e] == 0: H_e is not read -- NaN in unset memory does not survive.
 *   X        fp16 [R, n], row stride ldx >= n, a multiple of 8; 16-byte aligned.  Never written.
 *   offsets  int32 [E + 1], order int32 [P]: as qqq_moe_route writes them (the pairs sorted by expert).  order[] is followed AS GIVEN:
 *            it need not be ascending inside an expert, and the order is the summation order.
 *   a_div    >= 1: pair p is row p / a_div of X -- top_k where X holds one row per token (the inputs of gate | up), 1 where it holds one
 *            row per pair (the inputs of down).   R >= ceil(P / a_div).
 *   alpha, beta   f32 [E] in DEVICE memory: the running-mean factors differ per expert, and nothing is read on the host.
 *   n        a multiple of 64, 64 ... 32768;  1 <= E <= 256;  0 <= P <= 2097152 (P == 0: nothing is launched).
 *   H and X must be disjoint.
 *
 *   The bits: H_e is bit for bit what qqq_hessian_update(H_e, ldh, the c_e gathered rows as a contiguous matrix, c_e, n, alpha[e], beta[e])
 *   stores -- stages of 32 rows, the MFMA's own order within 16, one wave per entry, the epilogue's three roundings.  No atomics, no
 *   workspace, no split of the row loop; nothing depends on the strides, the stream or the run.
 *   Bounds: offsets are held inside [0, P] and ascending, a pair index inside [0, P), a row index inside [0, R), as qqq_moe_gemm holds
 *   them: garbage routing gives garbage matrices and never an access outside the arrays.
 *
 * Conventions are those of qqq_amd_hessian.h: ONE launch enqueued on `stream`, whose size depends on (E, n) alone -- a captured call
 * replays with another routing and gives the eager bits --, no allocation, no host sync, no state.  Return codes QQQ_OK (0) /
 * QQQ_ERR_ARG / QQQ_ERR_HIP with the values of include/qqq_amd.h, and a message in qqq_quant_last_error() (thread-local) that begins
 * with the entry's name; bad arguments -- n, E, P, a_div, R, the strides, alignment, overlap -- are rejected before any launch.
 */
#ifndef QQQ_AMD_HESSIAN_GROUPED_H_
#define QQQ_AMD_HESSIAN_GROUPED_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

int qqq_hessian_update_grouped(void* H, size_t lde, int ldh, const void* X, int ldx, const void* offsets, const void* order,
                               const void* alpha, const void* beta, int P, int R, int E, int n, int a_div, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_HESSIAN_GROUPED_H_ */
