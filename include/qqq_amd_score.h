/*
 * qqq_amd_score.h -- C-ABI of the fused scoring kernel (exported by libqqq_amd.so, beside include/qqq_amd.h and the other per-feature
 * headers): for every row of a batch of fp16 logits the log-probability of ONE target token under softmax(logits), and the row's argmax,
 * in ONE launch.  It is what perplexity and log-likelihood evaluation need from the logits, without an fp32 copy of them.
 *
 *   logits   fp16 [rows, vocab], row stride ld elements (ld >= vocab, ld % 8 == 0), 16-byte aligned; columns vocab ... ld-1 are never read
 *   targets  int64 [rows]       the token to score in each row
 *   logprob  f32 [rows], written
 *   argmax   int64 [rows], written; may be NULL (then it is not computed)
 *   1 <= vocab <= 262144, 0 <= rows <= 1048576; rows == 0 is a no-op (NULL pointers allowed).
 *
 * One row, with logits l_j and target t.  Key order, maximum and weights are the sampler's (include/qqq_amd_sample.h, items 3 and 6):
 *   1. order     NaN and -inf have no weight and are below every other value; -0 equals +0; +inf is a value like any other.
 *   2. argmax    the lowest index of the maximum logit; 0 in a row without any logit above -inf.  In every row that holds a finite logit it
 *                is the token qqq_sample_tokens returns at temperature 0.  (A row whose maximum is +inf and that holds no finite logit
 *                at all still reports that maximum's index here; the sampler returns 0 for it.)
 *   3. weights   exactly the sampler's at T = 1 without a cut: w_j = 1 for every logit equal to the maximum, otherwise
 *                exp2f((l_j - l_max) * log2 e) in f32, truncated to a multiple of 2^-44 (a weight below 2^-44 is 0).  They are summed as
 *                64-bit integers into W: the sum is exact and independent of its order, so a row's result does not depend on its row
 *                index, on ld, on how the row is split over waves, or on eager launch versus graph replay.
 *   4. result    logprob = (float)(((double)l_t - (double)l_max) - log((double)W * 2^-44)): the difference and the logarithm in f64, one
 *                rounding to f32 per row.  The target's own weight is not used, so a target far below the maximum, whose weight truncated
 *                to 0, still gets (l_t - l_max) - ln W.
 *   5. special targets, in this order:
 *                t < 0                      ignored, as with ignore_index: logprob = 0.0 (whatever the row holds)
 *                t >= vocab                 logprob = NaN: a bad label poisons a sum visibly
 *                no logit above -inf        logprob = NaN
 *                l_t NaN or -inf            logprob = -inf
 *   6. +inf      where +inf is the maximum its tie group has weight 1 each and every finite logit weight 0: a target in the group gets
 *                -log(count), a finite target -inf.
 *
 * One launch, one workgroup per row; the launch size depends on (rows, vocab) alone and nothing is read on the host, so a captured graph
 * replays with other contents of every array.  No workspace is needed.
 *
 * Conventions are those of include/qqq_amd.h: work only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state.
 * Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error() that begins with the entry's name; bad arguments
 * are rejected before any launch.
 * Alignment: logits 16 bytes; targets and argmax 8 bytes; logprob 4 bytes.
 */
#ifndef QQQ_AMD_SCORE_H_
#define QQQ_AMD_SCORE_H_

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int qqq_token_logprobs(const void* logits, int ld, const void* targets, void* logprob, void* argmax /* may be NULL */, int rows, int vocab,
                       int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_SCORE_H_ */
