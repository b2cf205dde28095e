/*
 * qqq_amd_factor.h -- C-ABI of the Cholesky factor op of the quantiser's library (libqqq_amd_quant.so; beside
 * qqq_amd_fakequant.h.  The prototypes and the ABI version of qqq_amd_quant.h stay as they are).  One device op: what GPTQ's
 * three-step chain  L = cholesky(H); Hi = cholesky_inverse(L); U = cholesky(Hi, upper)  computes, by the direct route.
 *
 * qqq_upper_factor   U = the upper triangular matrix with positive diagonal and U^T U = H^-1
 *   H      f32 [n, n], row stride ldh >= n in ELEMENTS and a multiple of 4; 16-byte aligned.  Symmetric positive-definite; only its
 *          upper triangle takes part in the result (the 64 x 64 tiles on the diagonal are fetched whole).  Never written.
 *   U      f32 [n, n], row stride ldu >= n, a multiple of 4; 16-byte aligned.  Receives the factor; its strict lower triangle is set to
 *          exact zeros (what torch.linalg.cholesky(upper=True) returns).  Nothing between the rows (columns n ... ldu - 1) is touched.
 *   n      a multiple of 64, 64 ... 32768 (QuantLinear's admission rule)
 *   work   device memory of qqq_upper_factor_work(n) bytes, 16-byte aligned: the running matrix [n, n] and a strip [n, 128].  Its
 *          contents need not be set and are unspecified afterwards.
 *   info   one device int32: 0, or 1 + the index of the first pivot that was <= 0 or NaN (LAPACK's convention; "first" in the order
 *          the pivots are taken, from column n - 1 down, so every pivot behind the reported one was positive).  After a failed pivot
 *          the rest of U is unspecified (NaN, as a rule); nothing is read or written out of bounds.
 *   H, U, work and info must be disjoint.
 *
 *   The route: with R = U^-1 (upper, positive diagonal), H = R R^T -- a Cholesky factorisation taken from the bottom-right corner
 *   upwards -- and U = R^-1: one factorisation and one triangular inverse, 2 n^3 / 3 flops, and no H^-1 in between.  It is the matrix
 *   the chain computes, as close to the exact one as the chain's own f32 result, not the chain's bits.
 *     blocks of 128 columns from the end (one first block of 64 where n is an odd multiple of 64); per block J, last to first:
 *       the diagonal block in one workgroup: column c from the last to the first, r_cc = sqrt(pivot), the column above scaled by
 *       1 / r_cc, r_ic * r_kc (rounded) subtracted from a_ik, i <= k < c; then its inverse by back-substitution: U_JJ
 *       the rows above: R_iJ = A_iJ . U_JJ^T, and the trailing update A_ik -= R_iJ . R_kJ^T, i <= k < J        (f32 MFMA tiles)
 *     then per block J, first to last:  U_{0:J, J} = - U_{0:J, 0:J} . (R_{0:J, J} . U_JJ)                      (f32 MFMA tiles)
 *   Every sum is taken in one fixed order by one workgroup, without atomics: U's bits depend on H's upper triangle and n alone, not on
 *   ldh / ldu, the stream, or the run.
 *
 * qqq_upper_factor_work   *bytes = the size of `work` for n.  Host only: no device, no launch.
 *
 * Conventions are those of qqq_amd_quant.h: work is only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no host
 * sync, no state; the launch sequence (about five launches per 128 columns) depends on n alone.  Return codes QQQ_OK (0) /
 * QQQ_ERR_ARG / QQQ_ERR_HIP with the values of include/qqq_amd.h, and a message in qqq_quant_last_error() (thread-local) that begins
 * with the entry's name; bad arguments -- n, strides below n or no multiple of 4, alignment, overlap -- are rejected before any launch.
 */
#ifndef QQQ_AMD_FACTOR_H_
#define QQQ_AMD_FACTOR_H_

#ifdef __cplusplus
extern "C" {
#endif

int qqq_upper_factor_work(int n, long long* bytes);
int qqq_upper_factor(const void* H, int ldh, void* U, int ldu, int n, void* work, void* info, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_FACTOR_H_ */
