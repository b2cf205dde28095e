/*
 * qqq_amd_rotate_k.h -- C-ABI of the rotation op for hidden sizes K * 2^p of the quantiser's library (libqqq_amd_quant.so; in
 * quant/include_ext/, beside quant/include/ with qqq_amd_quant.h, qqq_amd_gptq_order.h and qqq_amd_rotate.h, whose prototypes and ABI
 * version stay as they are: that directory's contents are pinned by name).  For a size that is
 * no power of two the reference's matmul_hadU multiplies by hadK (x) H_m: a K x K Hadamard matrix that mixes K sub-blocks, each turned
 * by the Sylvester matrix of m = 2^p.  This op does both in one launch; the K x K matrix is an ARGUMENT (the library ships none).
 *
 * qqq_hadamard_rows_k   Y[r, b*n : (b+1)*n] = (X[r, b*n : (b+1)*n] * sign) . (table^T (x) H_m) / d   for every row r and every block b
 *                       of n = K * m columns
 *   X, Y    [rows, cols], row-major, row strides ldx, ldy >= cols in ELEMENTS; dtype 0 = fp16, 1 = f32, shared by X and Y; both aligned
 *           to their element.  Y == X with ldy == ldx (in place) is allowed; any other overlap of the two is refused.
 *   K       a multiple of 4, 4 ... 64;  m a power of two, m >= 1;  n = K * m <= 8192;  cols % n == 0;  rows >= 1
 *   table   int8 [K, K], contiguous, in DEVICE memory: read by the kernel, never on the host.  Only whether an entry is negative is
 *           looked at; the caller checks that the entries are +-1 and that the matrix is Hadamard (table . table^T = K I).
 *   sign    NULL, or int8 [n] of +1 / -1 (the same for every block); only whether an entry is negative is looked at.
 *
 *   Per block, independently, in f64:
 *       v[i] = (double)x[i] * sign[i]                                                  (exact)
 *       per sub-block of m consecutive entries, for h = 1, 2, 4, ... m/2, for every i with (i & h) == 0:
 *           (v[i], v[i + h]) <- (v[i] + v[i + h], v[i] - v[i + h])                     (one f64 add each; none at m = 1)
 *       for k = 0 ... K-1 and c = 0 ... m-1, with s(k, k') = -1 where table[k][k'] < 0 and +1 otherwise:
 *           z = s(k, 0) * v[c];   for k' = 1 ... K-1:  z = z + s(k, k') * v[k' m + c]  (a sign flip and one f64 add per term,
 *           z[k m + c] = z                                                              k' ascending)
 *       y[j] = z[j] / d,   d = (double)sqrtf((float)n)                                 (one correctly rounded f64 divide)
 *   That is the reference's matmul_hadU for n = K * m with hadK = table: its butterflies in their order, then
 *   out[k, c] = sum_k' hadK[k][k'] in[k', c], and its divisor.  The index order matters: the reference's tables are not symmetric.
 *   y is stored rounded to f32, and for fp16 rounded to f32 and THEN to fp16, as qqq_hadamard_rows does.
 *
 *   Exactness.  fp16 inputs are multiples of 2^-24 of magnitude below 2^16.  Every partial sum of at most n <= 8192 of them is a
 *   multiple of 2^-24 of magnitude at most n * 65504 < 2^29: at most 53 significant bits, so every add of an fp16 block is exact in f64
 *   and the result is the exact sum divided and rounded.  For f32 inputs the sums round, and the order above is what fixes the bits.
 *
 *   A block's bits depend on that block, `sign` and `table` alone: not on rows, on the block's place in its row, or on the row's place
 *   in the launch (whether the 16-byte or the element-wise loads are taken changes no bit).
 *
 * Conventions are those of qqq_amd_quant.h: work is only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state,
 * one launch per call whose size depends on the shapes alone.  Return codes QQQ_OK (0) / QQQ_ERR_ARG / QQQ_ERR_HIP with the values of
 * include/qqq_amd.h, and a message in qqq_quant_last_error() (thread-local) that begins with the entry's name; bad arguments are
 * rejected before any launch.
 */
#ifndef QQQ_AMD_ROTATE_K_H_
#define QQQ_AMD_ROTATE_K_H_

#ifdef __cplusplus
extern "C" {
#endif

int qqq_hadamard_rows_k(const void* X, int ldx, void* Y, int ldy, int rows, int cols, int K, int m, const void* table, const void* sign,
                        int dtype, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_ROTATE_K_H_ */
