/*
 * qqq_amd_penalty.h -- C-ABI of the repetition / presence / frequency penalty (exported by libqqq_amd.so, beside include/qqq_amd.h and the
 * other per-feature headers): the logits of a batch are rewritten in place, conditioned on the tokens each row has seen, in ONE launch
 * that runs in front of a sampler (qqq_sample_tokens, qqq_sample_advance, qqq_spec_advance) and leaves the samplers as they are.  The
 * call also keeps the history it reads: it records every row's input token at the row's position.
 *
 *   logits       fp16  [rows * G, ld]         rewritten in place; G = group, 1 ... 16; ld >= vocab; columns vocab ... ld-1 are never touched
 *   ids          int64 [rows, G]              the forward's input tokens: [r, 0] the row's last token, [r, 1 ... G-1] its drafts
 *   pos          int64 [rows, G]              of which only pos[r, 0] is read: the sequence index of ids[r, 0]; [rows] at G = 1
 *   seen         int32 [rows, seen_stride]    the sequence so far, prompt and emitted tokens; seen[r, pos[r, 0]] is written
 *   n_prompt     int32 [rows]                 the prompt's length: sequence index i is a PROMPT index iff i < n_prompt[r], else an OUTPUT index
 *   repetition, presence, frequency  f32 [rows]
 *   workspace    qqq_penalize_logits_workspace_bytes(rows, vocab) bytes, 4-byte aligned, ZERO on entry and left ZERO on exit (one 32-bit
 *                word per row and vocabulary entry; allocate and clear it once, as the GEMM's lock workspace)
 *
 * One row r, with p = pos[r, 0]:
 *   p < 0 or p >= seen_stride    nothing of the row is read or written (an idle row of the loops, and a guard)
 *   otherwise, recording         seen[r, p] = ids[r, 0] if that lies in [0, vocab), else -1
 *   neutral row                  repetition[r] == 1, presence[r] == 0 and frequency[r] == 0 (exact compares): no logits row of r is written
 *   otherwise                    for j = 0 ... G-1, logits row r * G + j is conditioned on S_j = seen[r, 0 ... p] ++ ids[r, 1 ... j], the
 *                                draft ids[r, k] sitting at sequence index p + k.  Tokens outside [0, vocab) count for nothing.  For every
 *                                token t that occurs in S_j -- exactly once whatever its multiplicity -- with c = the number of its
 *                                occurrences at OUTPUT indices and x = f32(l_t):
 *                                  if repetition != 1:  x = x > 0 ? x / repetition : x * repetition
 *                                  if c > 0:            x = x - fl(frequency * f32(c)), then x = x - presence
 *                                  l_t = fp16(x), round to nearest even
 *                                Every operation is one correctly rounded f32 operation (no contraction into an FMA); every other entry
 *                                of the row keeps its bits.  NaN and +-inf need no special case: the arithmetic is carried out as written.
 *
 * The repetition rule is transformers' RepetitionPenaltyLogitsProcessor (over prompt and output), presence and frequency over the outputs
 * alone are vLLM's; all of them act before temperature, top-k and top-p because the call runs before the sampler.
 *
 * One launch, one workgroup per row, O(p + G) work per row and not O(vocab): the lanes scatter the history into the row's workspace
 * words with integer atomics (bit 31: a prompt occurrence; the low bits: the output occurrences), one lane per token collects the final
 * word -- clearing it -- and applies the rule.  What is applied depends on the final counts alone, so the result is reproducible to the
 * bit although the arrival order is not.  The launch size depends on (rows, G, vocab, seen_stride) alone and nothing is read on the host,
 * so a captured graph replays with other contents of every array.
 *
 * Conventions are those of include/qqq_amd.h: work only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state.
 * Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error() that begins with the entry's name; bad arguments
 * are rejected before any launch: rows in [0, 65535], 1 <= group <= 16, rows * group <= 65535, 1 <= vocab <= 262144, ld >= vocab,
 * seen_stride >= 1, every pointer non-NULL, logits 2-byte, ids and pos 8-byte and everything else 4-byte aligned, workspace_bytes at least
 * what qqq_penalize_logits_workspace_bytes returns.  rows == 0 is a no-op (NULL pointers allowed).
 */
#ifndef QQQ_AMD_PENALTY_H_
#define QQQ_AMD_PENALTY_H_

#include <stddef.h>

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of `workspace` for a call with these rows and vocab; 0 for arguments the call rejects */
size_t qqq_penalize_logits_workspace_bytes(int rows, int vocab);

int qqq_penalize_logits(void* logits, int ld, const void* ids, const void* pos, int group, void* seen, int seen_stride,
                        const void* n_prompt, const void* repetition, const void* presence, const void* frequency, void* workspace,
                        size_t workspace_bytes, int rows, int vocab, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_PENALTY_H_ */
