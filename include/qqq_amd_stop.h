/*
 * qqq_amd_stop.h -- C-ABI of the two device ops behind generate()'s `stop`, `stop_token_ids` and `min_new_tokens` (exported by
 * libqqq_amd.so, beside include/qqq_amd.h and the other per-feature headers): the ways a completion ends besides its budget and its one
 * eos id, decided where eos is decided -- on the device, inside a decode loop's captured step.  All of it is integer work.
 *
 * qqq_ban_tokens runs in FRONT of a sampler and rewrites fp16 logits in place: the minimum length.
 *   logits        fp16 [rows * G, vocab], row stride ld elements (ld >= vocab), 2-byte aligned, rewritten in place
 *   n_out         int32 [rows]   a row's count of emitted tokens;  base  a scalar added to it
 *   min_new       int32 [rows]   the row's minimum length M;  eos  int32 [rows]  the row's eos id, -1 for none
 *   ban_ids       int32 [n_ban]  further ids (the stop token ids), shared by the rows; 0 <= n_ban <= 32, NULL exactly when n_ban == 0
 *   1 <= G <= 16, rows * G <= 65535, 1 <= vocab <= 262144
 *   Logits row r * G + j is the row the completion's token of index n_out[r] + base + j (0-based) is drawn from.  If that index is
 *   < min_new[r], logits[row, eos[r]] and logits[row, ban_ids[i]] for every i become fp16 -inf (0xFC00); ids outside [0, vocab) are
 *   ignored, duplicates are fine.  Every other entry keeps its bits, the columns vocab ... ld-1 included.  The decode loops call it with
 *   base = 1 (the prefill's token is index 0 of the completion and n_out does not count it), admission and the host path with base = 0
 *   and their own counts.
 *
 * qqq_stop_check runs BEHIND qqq_sample_advance / qqq_spec_advance (include/qqq_amd_step.h, qqq_amd_spec.h) and ends a row whose
 * completion has run into a stop sequence or a stop token id.
 *   The completion c_r of row r has m = n_out[r] + 1 tokens and is addressed through (tokens, token_bytes, tok_stride, base, first):
 *   tokens        int32 (token_bytes 4) or int64 (token_bytes 8) [rows, tok_stride];  base  int32 [rows];  first  int32 [rows] or NULL
 *   c_r[i] is first[r] if base[r] + i < 0, else tokens[r, base[r] + i]; an index at or beyond tok_stride, or below 0 with first NULL,
 *   holds no token and equals nothing.  The decode loop passes its `out` (int64) with base -1 and first = the prefill's token, the
 *   speculative loop its `hist` (int32) with base = the prompt's length.
 *   stop_ids      int32 [n_stop, stop_stride], stop_len int32 [n_stop]: sequence s is stop_ids[s, 0 ... stop_len[s]); a length outside
 *                 [1, stop_stride] is an unused entry.  0 <= n_stop <= 32, 1 <= stop_stride <= 32; both NULL exactly when n_stop == 0
 *   end_ids       int32 [n_end]: the stop token ids (an entry < 0 is unused); 0 <= n_end <= 32, NULL exactly when n_end == 0
 *   eos           int32 [rows] or NULL: the row's eos id (-1 for none), what qqq_sample_advance / qqq_spec_advance retired the row on
 *   min_new       int32 [rows];  n_seen  int32 [rows]: the length up to which the row has been checked, updated in place
 *   n_trim, stop_hit   int32 [rows], written on a match alone
 *   ids, pos, slots    int64 [rows, G];  start  int64 [rows] or NULL;  remaining  int32 [rows]: the row state to retire, 1 <= G <= 16
 *   Per row, with a = max(n_seen[r], 0): if a >= m the row writes nothing at all (an idle row, a row that emitted nothing).  Otherwise the
 *   ends e = a + 1 ... m are tested in ascending order:
 *     0. c_r[e - 1] == eos[r] >= 0 matches: the token stays, trim = m - e, hit = n_stop + n_end;
 *     1. else an end id i with c_r[e - 1] == end_ids[i] matches: the token stays, trim = m - e, hit = n_stop + i;
 *     2. else, if e >= min_new[r], a stop sequence s with 1 <= L_s <= e and c_r[e - L_s ... e) == stop_ids[s, 0 ... L_s) matches: the
 *        completion is cut in front of it, trim = m - e + L_s, hit = s.
 *   The earliest e wins; at one e the eos goes first, then the end ids, then the sequences, among each the lowest index.  So a completion
 *   that ends in its eos or in a stop id keeps that token even where a stop sequence ends in the same token, as the host path has it.
 *   (eos and the end ids are tested below min_new too: qqq_ban_tokens keeps them from being drawn there.)  On a match n_trim[r] = trim,
 *   stop_hit[r] = hit and the row retires as in include/qqq_amd_step.h / qqq_amd_spec.h: ids 0, pos / slots -1 for its G entries, start -1
 *   (if given), remaining 0.  In every case n_seen[r] = m.  A row that its eos or its budget retired in the same step is still checked.
 *   The caller drops the last n_trim[r] tokens of the completion; it sets n_seen = 1 and n_trim = 0 when it admits a sequence, having
 *   checked the first token itself.
 *
 * One launch each; the launch size depends on (rows, G) alone and nothing is read on the host, so a captured graph replays with other
 * contents of every array.  No workspace.  Conventions are those of include/qqq_amd.h: work only ENQUEUED on `stream` (safe under
 * hipGraph capture), no allocation, no state.  Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error()
 * that begins with the entry's name; bad arguments are rejected before any launch.  rows == 0 is a no-op (NULL pointers allowed),
 * 0 <= rows <= 65535.
 * Alignment: logits 2 bytes; tokens token_bytes; ids, pos, slots and start 8 bytes; everything else 4 bytes.
 */
#ifndef QQQ_AMD_STOP_H_
#define QQQ_AMD_STOP_H_

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int qqq_ban_tokens(void* logits, int ld, const void* n_out, int base, const void* min_new, const void* eos,
                   const void* ban_ids /* NULL iff n_ban == 0 */, int n_ban, int group, int rows, int vocab, int dev, void* stream);

int qqq_stop_check(const void* tokens, int token_bytes, int tok_stride, const void* base, const void* first /* may be NULL */,
                   const void* n_out, const void* stop_ids, int stop_stride, const void* stop_len, int n_stop,
                   const void* end_ids /* NULL iff n_end == 0 */, int n_end, const void* eos /* may be NULL */, const void* min_new,
                   void* n_seen, void* n_trim, void* stop_hit, void* ids, void* pos, void* slots, void* start /* may be NULL */,
                   void* remaining, int group, int rows, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_STOP_H_ */
