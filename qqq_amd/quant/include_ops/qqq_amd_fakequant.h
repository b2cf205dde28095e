/*
 * qqq_amd_fakequant.h -- C-ABI of the fake-quantisation op of the quantiser's library (libqqq_amd_quant.so; in quant/include_ops/, the
 * third flat header directory of the quantiser: the contents of quant/include/ and quant/include_ext/ are pinned by name, so this and
 * every later quantiser op's header go here.  The prototypes and the ABI version of qqq_amd_quant.h stay as they are).  One device op:
 * what the reference's smoothing search (QQQ/smooth/migration, MigratorBase.quantize) spends about fourteen elementwise and reduction
 * launches on per operand and candidate.  Everything else of smoothing is plain torch in qqq_amd/quant/smooth.py.
 *
 * qqq_fake_quant_rows   Y = fake_quant(X op col_scale): symmetric, `bits` wide, one scale per row or per (row, group of 128 columns)
 *   X, Y       fp16 [rows, cols], row-major, row strides ldx, ldy >= cols in ELEMENTS and multiples of 8; both 16-byte aligned.
 *              Y == X with ldy == ldx (in place) is allowed; any other overlap of the two is refused.
 *   rows >= 1;  cols a multiple of 8, 8 ... 2^30
 *   col_scale  NULL, or fp16 [cols], contiguous, 16-byte aligned, in device memory
 *   bits       8 or 4: qmax = 2^(bits-1) - 1 = 127 or 7
 *   group      0: one scale per row.  128: one scale per (row, 128 consecutive columns); cols % 128 == 0
 *   divide     1: t = x / col_scale (the activation side).  0: t = x * col_scale (the weight side).  Ignored when col_scale is NULL.
 *
 *   Per row (group 0) or per group of 128 columns of a row (group 128), independently; every line is ONE f32 operation on fp16 values
 *   whose result is rounded to fp16 (round to nearest even, subnormals kept) -- what torch stores for an fp16 elementwise op:
 *       t[j] = fp16(f32(x[j]) op f32(col_scale[j]))              op is / or *;  t[j] = x[j] when col_scale is NULL
 *       a    = max(-min(min_j t[j], 0), max(max_j t[j], 0))      exact
 *       s    = max(fp16(f32(a) / qmax), 2^-23)                   2^-23 = fp16(1.1920929e-07), an fp16 subnormal: the reference's eps
 *       r[j] = rint(fp16(f32(t[j]) / f32(s)))                    half to even; a result of -0 becomes +0
 *       r[j] = min(max(r[j], -qmax), qmax)
 *       y[j] = fp16(f32(r[j]) * f32(s))
 *   The divides are correctly rounded.  No y is -0.  An all-zero row gives zeros (s = 2^-23).  Rows that hold a NaN or an infinity
 *   (or reach one through col_scale) give unspecified values; nothing is read or written out of bounds for them.
 *
 *   A row's bits depend on that row and col_scale alone: not on rows, on ldx / ldy, or on the row's place in the launch (rows of at
 *   most 16384 columns are read once and kept in registers, wider rows are read twice; the bits are the same).
 *
 * Conventions are those of qqq_amd_quant.h: work is only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state,
 * one launch per call whose size depends on the shapes alone.  Return codes QQQ_OK (0) / QQQ_ERR_ARG / QQQ_ERR_HIP with the values of
 * include/qqq_amd.h, and a message in qqq_quant_last_error() (thread-local) that begins with the entry's name; bad arguments are
 * rejected before any launch.
 */
#ifndef QQQ_AMD_FAKEQUANT_H_
#define QQQ_AMD_FAKEQUANT_H_

#ifdef __cplusplus
extern "C" {
#endif

int qqq_fake_quant_rows(const void* X, int ldx, void* Y, int ldy, int rows, int cols, const void* col_scale, int bits, int group,
                        int divide, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_FAKEQUANT_H_ */
