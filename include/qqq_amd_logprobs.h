/*
 * qqq_amd_logprobs.h -- C-ABI of the fused top-k log-probability kernel (exported by libqqq_amd.so, beside include/qqq_amd.h and
 * the other per-feature headers): for every row of a batch of fp16 logits the log-probability and the rank of ONE token, and the k most probable
 * tokens with their log-probabilities, in ONE launch.  It is what OpenAI-style `logprobs` / `top_logprobs` need from the logits a sampler
 * drew from, without an fp32 copy of them and without a sort of the vocabulary.
 *
 *   logits        fp16 [rows, vocab], row stride ld elements (ld >= vocab, ld % 8 == 0), 16-byte aligned; columns vocab ... ld-1 are never read
 *   tokens        int64 [rows]       the token to score in each row; NULL together with logprob and rank: only the top-k part is computed
 *   logprob       f32 [rows], written;  rank  int32 [rows], written
 *   top_ids       int32 [rows, k], written;  top_logprobs  f32 [rows, k], written; both NULL exactly when k == 0
 *   0 <= k <= 32 and k <= vocab; 1 <= vocab <= 262144, 0 <= rows <= 65535; rows == 0 is a no-op (NULL pointers allowed).  A call that asks
 *   for neither part (tokens NULL and k == 0) is refused.
 *
 * One row, with logits l_j, the token t and k.  Key order and weights are the sampler's (include/qqq_amd_sample.h), a value is the
 * scorer's (include/qqq_amd_score.h) to the bit:
 *   1. order     NaN and -inf are below every other value and equal among themselves; -0 equals +0; +inf is a value like any other.
 *   2. logprob   what qqq_token_logprobs returns for (row, t): t < 0 gives 0.0, t >= vocab NaN, a row without a logit above -inf NaN, a
 *                token whose logit is NaN or -inf gives -inf; W is the exact integer sum of the fixed-point weights, the logarithm is
 *                taken in f64 and the result rounded to f32 once.
 *   3. rank      1 + the number of tokens whose logit is above l_t in the order of 1, for 0 <= t < vocab; otherwise 0.  Ties share a rank.
 *   4. top-k     the first k tokens in the order (logit descending, index ascending), written in that order; top_logprobs[i] is the
 *                value logprob has for top_ids[i].  Entry 0 is qqq_token_logprobs' argmax, and qqq_sample_tokens' token at temperature 0
 *                in every row that holds a finite logit.  Ties at the cut are resolved exactly: the lowest indices enter, however many
 *                tokens tie and wherever they sit.  A row with fewer than k logits above -inf goes on with its NaN / -inf tokens in
 *                index order, at -inf each (NaN each in a row without any logit above -inf, whose ids are 0 ... k-1).
 *
 * qqq_topk_logprobs_step is the decode loop's epilogue, run behind qqq_sample_advance (include/qqq_amd_step.h) on the logits that call
 * drew from:
 *   out           int64 [rows, out_stride], n_out int32 [rows]: that call's emitted tokens and their number, only read
 *   n_rec         int32 [rows]: the records a row has so far, updated in place
 *   logprob / rank              f32 / int32 [rows, cap];  top_ids / top_logprobs  int32 / f32 [rows, cap, k] (NULL exactly when k == 0)
 *   With a = n_rec[r] and b = n_out[r]: if 0 <= a < b and a < cap, the row's token is out[r, a], its results go to record (r, a) of the
 *   four arrays and n_rec[r] becomes a + 1.  Otherwise the row writes nothing and n_rec[r] is untouched: an idle row, a row that emitted
 *   nothing in this step, a row without room.  A row writes at most one record per call; n_rec[r] is read and written by the row's own
 *   workgroup alone.  The host resets n_rec[r] together with n_out[r] when it admits a sequence into the row.
 *
 * One launch, one workgroup per row; the launch size depends on (rows, vocab, k) alone and nothing is read on the host, so a captured
 * graph replays with other contents of every array.  A row's results do not depend on its row index, on ld, or on eager launch versus
 * graph replay.  No workspace is needed.
 *
 * Conventions are those of include/qqq_amd.h: work only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state.
 * Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error() that begins with the entry's name; bad arguments
 * are rejected before any launch.
 * Alignment: logits 16 bytes; tokens and out 8 bytes; everything else 4 bytes.
 */
#ifndef QQQ_AMD_LOGPROBS_H_
#define QQQ_AMD_LOGPROBS_H_

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int qqq_topk_logprobs(const void* logits, int ld, const void* tokens /* may be NULL */, void* logprob, void* rank, void* top_ids,
                      void* top_logprobs, int k, int rows, int vocab, int dev, void* stream);

int qqq_topk_logprobs_step(const void* logits, int ld, const void* out, int out_stride, const void* n_out, void* n_rec, void* logprob,
                           void* rank, void* top_ids, void* top_logprobs, int cap, int k, int rows, int vocab, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_LOGPROBS_H_ */
