/*
 * qqq_amd_hessian.h -- C-ABI of the Hessian accumulation op of the quantiser's library (libqqq_amd_quant.so; beside
 * qqq_amd_fakequant.h and qqq_amd_factor.h.  The prototypes and the ABI version of qqq_amd_quant.h stay as they are).  One device op:
 * what GPTQ's add_batch does to its running Hessian per calibration batch, as one symmetric rank-k launch on the fp16 matrix path.
 *
 * qqq_hessian_update   H[i][j] <- f32( f32(alpha * H[i][j]) + f32(beta * S[i][j]) )  for EVERY i, j < n,  S = sum_t X[t][i] * X[t][j]
 *   H      f32 [n, n], row stride ldh >= n in ELEMENTS and a multiple of 4; 16-byte aligned.  The whole symmetric matrix is written, not a
 *          triangle, every entry from its own old value; S[i][j] and S[j][i] are one sum, so a symmetric H stays bit-symmetric.  Nothing
 *          between the rows (columns n ... ldh - 1) is touched.
 *          alpha == 0: H is not read at all -- the first call may take unset memory, and NaN in it does not survive.
 *   X      fp16 [tokens, n], row stride ldx >= n, a multiple of 8; 16-byte aligned.  Never written.
 *   tokens >= 1, no multiple of anything: the rows beyond the last count as zeros.
 *   n      a multiple of 64, 64 ... 32768 (QuantLinear's admission rule, as qqq_upper_factor)
 *   H and X must be disjoint.
 *
 *   The arithmetic: a product of two fp16 values is exact in f32; the sum over t is taken in f32 (v_mfma_f32_32x32x16_f16, sixteen
 *   tokens an instruction, the tokens ascending in steps of 16) by ONE wave per entry in one order that depends on `tokens` and n alone --
 *   no atomics, no split of the token loop, no workspace -- so the bits do not depend on ldh / ldx, the stream, or the run.  The epilogue
 *   rounds the two products and their sum one by one (the library is built without floating-point contraction).
 *
 * Conventions are those of qqq_amd_factor.h: work is only ENQUEUED on `stream` (safe under hipGraph capture: a replay gives the eager
 * bits), one launch, no allocation, no host sync, no state.  Return codes QQQ_OK (0) / QQQ_ERR_ARG / QQQ_ERR_HIP with the values of
 * include/qqq_amd.h, and a message in qqq_quant_last_error() (thread-local) that begins with the entry's name; bad arguments -- n,
 * tokens < 1, strides below n or no multiple of 4 / 8, alignment, overlap -- are rejected before any launch.
 */
#ifndef QQQ_AMD_HESSIAN_H_
#define QQQ_AMD_HESSIAN_H_

#ifdef __cplusplus
extern "C" {
#endif

int qqq_hessian_update(void* H, int ldh, const void* X, int ldx, int tokens, int n, float alpha, float beta, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_HESSIAN_H_ */
