/*
 * qqq_amd_lora.h -- C-ABI of the batched LoRA op (exported by libqqq_amd.so, beside include/qqq_amd.h and the other
 * per-feature headers): low-rank fp16 adapters added beside the W4A8 GEMM, several adapters mixed in one batch, the adapter of every
 * token read from device memory.
 *
 * qqq_lora_add
 *   y          fp16 [T, N], row stride ldy elements (ldy >= N, even), 4-byte aligned, updated in place: the GEMM's output, bias included
 *   xq         int8 [T, K] contiguous, 16-byte aligned;  s1  f32 [T]: the quantised activation the GEMM consumed, x^ = s1 * xq
 *   A          fp16 [S, P * R, K]: rows and columns contiguous, slot stride a_stride elements (>= P * R * K, a multiple of 8), 16-byte aligned
 *   B          fp16 [S, N, R]:     rows and columns contiguous, slot stride b_stride elements (>= N * R, a multiple of 8), 16-byte aligned
 *   scale      f32 [S];  slot  int32 [T] in device memory, -1: no adapter
 *   part_cols  int [P + 1] in HOST memory (the one pointer of the call that is read on the host): ascending column offsets from 0 to N,
 *              every entry a multiple of 64.  Column n of part p (part_cols[p] <= n < part_cols[p + 1]) uses the rows p * R ...
 *              (p + 1) * R - 1 of A, so one call serves q|k|v or gate|up on their shared input.
 *   For a row t with a = slot[t] in [0, S) and a column n of part p
 *       y[t, n] <- fp16( float(y[t, n]) + scale[a] * sum_r B[a, n, r] * ( s1[t] * sum_k A[a, p * R + r, k] * xq[t, k] ) )
 *   with every product and sum at f32 precision or better and one rounding to fp16 at the end; the intermediate [T, P * R] never leaves
 *   the chip.  A row whose slot is outside [0, S) -- -1 or any other value -- is not written at all: it keeps its bits, and the index is
 *   never turned into an address.
 *   The bits of row t depend on row t's own y, xq, s1 and its slot's matrices alone: not on T, on the row's place in the batch or on the
 *   other rows' slots (no float atomics, one arithmetic for every T); and a call with P parts gives the bits of P calls with one part on
 *   the column slices, with the matching views of A and B.
 *
 * One launch; the launch size depends on (T, N, K, R, P, part_cols) alone and nothing is read on the host but part_cols, so a captured
 * graph replays with other contents of every array -- other slots and other adapters in the same buffers included.  No workspace.
 * Conventions are those of include/qqq_amd.h: work only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state.
 * Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error() that begins with the entry's name; bad arguments
 * are rejected before any launch.  T == 0 is a no-op (NULL pointers allowed).
 * Limits: 0 <= T <= 1048576, N and K multiples of 64 (QuantLinear's admission rule), R in {8, 16, 32, 64}, 1 <= P <= 3, S >= 1.
 */
#ifndef QQQ_AMD_LORA_H_
#define QQQ_AMD_LORA_H_

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int qqq_lora_add(void* y, int ldy, const void* xq, const void* s1, const void* A, size_t a_stride, const void* B, size_t b_stride,
                 const void* scale, const void* slot, const void* part_cols /* host */, int P, int T, int N, int K, int R, int S, int dev,
                 void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_LORA_H_ */
