/*
 * qqq_amd_beam.h -- C-ABI of beam search on the device (exported by libqqq_amd.so, beside include/qqq_amd.h and the other per-feature
 * headers): the step that follows a pass's logits, and the block
 * copies of a cache reorder.
 *
 * qqq_beam_step: P prompts of B = num_beams beams each; row p * B + b of every per-row array is beam b of prompt p.
 *   logits        fp16 [P * B, vocab], row stride ld elements (ld >= vocab, ld % 8 == 0), 16-byte aligned; columns vocab ... ld-1 never read
 *   cum           f32 [P * B]    the beams' summed log-probabilities
 *   live          int32 [P * B]  a row with 0 contributes nothing and its logits are never read: the rows 1 ... B-1 of the first pass behind
 *                                a prefill, the rows of a prompt that is done
 *   1 <= num_beams <= 16 (k = 2B <= 32, qqq_topk_logprobs' bound); eos: the id that ends a hypothesis, -1 for none;
 *   2B <= vocab <= 262144; rows = P * B, a multiple of B, 0 <= rows <= 65535; rows == 0 is a no-op (NULL pointers allowed).
 *
 * One prompt (this is the definition; tests/beam_ref.py restates it in numpy):
 *   1. every live row yields its first 2B tokens in the order of qqq_topk_logprobs' rule 4 (include/qqq_amd_logprobs.h), with that
 *      entry's top_logprobs to the bit.
 *   2. a candidate is (b, i): the token ids[i] of row b, lp = top_logprobs[i], score = cum[row] + lp as ONE f32 addition.
 *   3. candidates are ordered by score descending -- NaN and -inf are equal and below everything, -0 equals +0, as in the key order --
 *      then by b ascending, then by i ascending.  The first 2B are written to cand_score f32, cand_logprob f32, cand_parent int32 (b) and
 *      cand_token int32, each [P, 2B].  A prompt with a live row always has at least 2B candidates; a prompt without one writes
 *      parent = token = -1 and score = logprob = -inf.
 *   4. walking those 2B in order, a candidate whose token is eos is a finish -- the caller counts it only at a position < B (transformers'
 *      rule) and reads it off cand_token; the kernel only leaves it out of what follows.  The first B candidates whose token is not eos
 *      become the next beams 0 ... B-1.  At least B exist: a live beam contributes eos at most once.
 *   5. for the next beams: next_ids int64 [P * B] (the next pass's input, which need not leave the device), next_parent int32 [P * B] (b),
 *      next_cum f32 [P * B] (score), next_live int32 [P * B] (1).  A prompt without a live row writes ids 0, parent -1, cum -inf, live 0.
 *
 * TWO launches on `stream`, one behind the other, and a workspace: one workgroup per row writes the row's 2B candidates (rule 1) into the
 * workspace, then one wave per prompt merges them (rules 2 - 5).  The launch sizes depend on (rows, num_beams, vocab) alone and nothing is
 * read on the host -- no host sync -- so a captured graph replays with other contents of every array.  A prompt's results do not depend on
 * its index, on ld, or on eager launch versus replay.  The WORKSPACE has qqq_beam_step_workspace_bytes(rows, num_beams) bytes (0 for
 * arguments the entry refuses), 4-byte aligned: int32 and f32 [P * B, 2B].  Its contents on entry do not matter and mean nothing
 * afterwards; calls in flight at once on different streams need a workspace each.
 *
 * qqq_copy_blocks: the partial-block copies of a whole cache reorder in one launch.
 *   pools         a DEVICE array of n_pools base pointers; every pool is [num_blocks] blocks of block_bytes bytes (a multiple of 16), its
 *                 base 16-byte aligned (a pool whose base is not copies nothing)
 *   src, dst      int32 [n], device: block src[j] is copied to block dst[j] in every pool, with 16-byte accesses.  The dst entries are
 *                 distinct and none equals a src entry; one src may feed several dst.  An id outside [0, num_blocks) copies nothing.
 *   n == 0 is a no-op (NULL pointers allowed); 0 <= n <= 1048560, 1 <= n_pools <= 65535.
 * One launch of n * n_pools workgroups; nothing is read on the host.
 *
 * Conventions are those of include/qqq_amd.h: work only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state.
 * Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error() that begins with the entry's name; bad arguments
 * are rejected before any launch.
 * Alignment: logits 16 bytes; next_ids and pools 8 bytes; everything else 4 bytes.
 */
#ifndef QQQ_AMD_BEAM_H_
#define QQQ_AMD_BEAM_H_

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t qqq_beam_step_workspace_bytes(int rows, int num_beams);

int qqq_beam_step(const void* logits, int ld, const void* cum, const void* live, void* cand_score, void* cand_logprob, void* cand_parent,
                  void* cand_token, void* next_ids, void* next_parent, void* next_cum, void* next_live, void* workspace,
                  size_t workspace_bytes, int num_beams, int eos, int rows, int vocab, int dev, void* stream);

int qqq_copy_blocks(const void* pools, int n_pools, const void* src, const void* dst, int n, size_t block_bytes, int num_blocks, int dev,
                    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_BEAM_H_ */
