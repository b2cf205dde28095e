/*
 * qqq_amd_sample.h -- C-ABI of the fused token sampler (exported by libqqq_amd.so, beside include/qqq_amd.h and the other per-feature
 * headers): logits to next-token ids for a whole batch in ONE launch -- temperature, top-k, top-p and the draw, with every per-row
 * parameter and the uniform variate read from device memory.
 *
 *   logits       fp16 [rows, vocab], row stride ld elements (ld >= vocab, ld % 8 == 0), 16-byte aligned; columns vocab ... ld-1 are never read
 *   temperature  f32 [rows]       top_k  int32 [rows]       top_p  f32 [rows]       u  f32 [rows]: one uniform variate per row
 *   tokens       int64 [rows], written
 *   1 <= vocab <= 262144, rows <= 65535; rows == 0 is a no-op (NULL pointers allowed).
 *
 * One row, with logits l_j, temperature T, top-k k, top-p p:
 *   1. greedy    T <= 0, T NaN or k == 1: the lowest index of the maximum logit.  Nothing below applies.
 *   2. top-k     k <= 0 or k >= vocab keeps every token; otherwise the tokens with l_j >= the k-th largest logit VALUE are kept -- ties at
 *                that value all stay (transformers' TopKLogitsWarper, which removes scores < kth).
 *   3. weights   w_j = exp((l_j - l_max) / T) over the kept tokens, W their sum.  Computed in f32 (the maximum's weight is exactly 1), then
 *                truncated to a multiple of 2^-44 and summed as integers: every sum below is exact and independent of the order it is
 *                formed in, so a call is reproducible to the bit.  A weight below 2^-44 is 0.
 *   4. top-p     p >= 1 or p NaN keeps the top-k set; otherwise token j stays iff the mass of the kept tokens no more probable than it exceeds
 *                (1 - p) W:  sum of w_i over l_i <= l_j  >  (1 - p) * W.  The tie group of the maximum always stays (p <= 0 leaves it alone).
 *                This is TopPLogitsWarper, except that equal logits at the cut are kept or dropped together.
 *   5. draw      u is clamped into [0, 1) (NaN and negatives to 0, 1 and above to the largest f32 below 1).  With c_j the running sum of w
 *                over the surviving tokens in token-id order and W2 its total, the result is the lowest surviving j with c_j > u * W2
 *                (u * W2 in f64, rounded down).  The sums being exact, such a j always exists.
 *   6. special   -inf and NaN logits have weight 0 and count as the smallest values for top-k.  -0 equals +0.  +inf is a value like any
 *                other: where it is the maximum, its tie group has weight 1 and every finite logit weight 0.  A row without a finite logit
 *                returns 0.  Whatever the bits of the logits and the parameters, the result lies in [0, vocab).
 *
 * One launch, one workgroup per row; the launch size depends on (rows, vocab) alone and nothing is read on the host, so a captured graph
 * replays with other contents of every array.  No workspace is needed.
 *
 * Conventions are those of include/qqq_amd.h: work only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state.
 * Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error() that begins with the entry's name; bad arguments
 * are rejected before any launch.
 * Alignment: logits 16 bytes; tokens 8 bytes; temperature, top_k, top_p and u 4 bytes.
 */
#ifndef QQQ_AMD_SAMPLE_H_
#define QQQ_AMD_SAMPLE_H_

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int qqq_sample_tokens(const void* logits, int ld, const void* temperature, const void* top_k, const void* top_p, const void* u,
                      void* tokens, int rows, int vocab, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_SAMPLE_H_ */
