/*
 * qqq_amd_rotate.h -- C-ABI of the rotation op of the quantiser's library (libqqq_amd_quant.so, beside qqq_amd_quant.h, whose four
 * prototypes and ABI version stay as they are).  One device op: the blocked Walsh-Hadamard transform of matrix rows, what the
 * reference's rotation (QQQ/rotation) spends f64 matmuls by a Hadamard matrix and a CUDA package on.  Everything else of rotation is
 * plain torch in qqq_amd/quant/rotation.py.
 *
 * qqq_hadamard_rows   Y[r, b*n : (b+1)*n] = (X[r, b*n : (b+1)*n] * sign) . H_n / d   for every row r and every block b of n columns
 *   X, Y    [rows, cols], row-major, row strides ldx, ldy >= cols in ELEMENTS; dtype 0 = fp16, 1 = f32, shared by X and Y; both aligned
 *           to their element.  Y == X with ldy == ldx (in place) is allowed; any other overlap of the two is refused.
 *   n       a power of two, 2 ... 8192;  cols % n == 0;  rows >= 1
 *   sign    NULL, or int8 [n] of +1 / -1 (the diagonal of a randomised Hadamard matrix; the same for every block).  The caller
 *           checks that the entries are +-1: only whether an entry is negative is looked at.
 *
 *   Per block, independently, in f64:
 *       v[i] = (double)x[i] * sign[i]                                          (exact)
 *       for h = 1, 2, 4, ... n/2, for every i with (i & h) == 0:
 *           (v[i], v[i + h]) <- (v[i] + v[i + h], v[i] - v[i + h])             (one f64 add each)
 *       y[j] = v[j] / d,   d = (double)sqrtf((float)n)                         (one correctly rounded f64 divide)
 *   That is the natural-order Sylvester matrix H[i][j] = (-1)^popcount(i & j), the one the reference's matmul_hadU builds, and its
 *   divisor (an f32 square root promoted to f64: exact scaling when n is a power of 4).  y is stored rounded to f32, and for fp16
 *   rounded to f32 and THEN to fp16: the double rounding of torch's f64 -> fp16 conversion, which the reference's .to(dtype) performs.
 *
 *   Exactness.  fp16 inputs are multiples of 2^-24 of magnitude below 2^16.  After any number of stages every value is a multiple of
 *   2^-24 of magnitude at most n * 65504 < 2^13 * 2^16 = 2^29 for n <= 8192, so it has at most 29 + 24 = 53 significant bits: every
 *   stage of an fp16 block is exact in f64, and the result is the exact sum divided and rounded.  For f32 inputs the sums round, and
 *   the stage order above (h ascending, one add per output) is what fixes the bits.
 *
 *   A block's bits depend on that block and `sign` alone: not on rows, on the block's place in its row, or on the row's place in the
 *   launch (whether the 16-byte or the element-wise loads are taken changes no bit).
 *
 * Conventions are those of qqq_amd_quant.h: work is only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state,
 * one launch per call whose size depends on the shapes alone.  Return codes QQQ_OK (0) / QQQ_ERR_ARG / QQQ_ERR_HIP with the values of
 * include/qqq_amd.h, and a message in qqq_quant_last_error() (thread-local) that begins with the entry's name; bad arguments are
 * rejected before any launch.
 */
#ifndef QQQ_AMD_ROTATE_H_
#define QQQ_AMD_ROTATE_H_

#ifdef __cplusplus
extern "C" {
#endif

int qqq_hadamard_rows(const void* X, int ldx, void* Y, int ldy, int rows, int cols, int n, const void* sign, int dtype, int dev,
                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_ROTATE_H_ */
