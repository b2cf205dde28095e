/*
 * qqq_amd_spec.h -- C-ABI of the speculative decode loop's verify-and-advance step (exported by libqqq_amd.so, beside include/qqq_amd.h and
 * the other per-feature headers).  A row of the loop feeds its last emitted token and K = draft_len guessed tokens ("drafts") through one
 * forward pass; this call draws a token from each of the row's G = K + 1 logits rows with the ordinary sampler, keeps the draws whose
 * prefix was guessed right, appends them to the row's history, drafts the next K tokens from that history by n-gram lookup, and moves the
 * row to its next positions and cache slots or retires it -- all on the device, so that forward + this call is one graph replayed many
 * times between host syncs, as with qqq_sample_advance (include/qqq_amd_step.h), emitting 1 ... G tokens per row and replay.
 *
 * Per-row state of `rows` rows, all in device memory:
 *   logits       fp16  [rows * G, ld]         draw j of row r reads logits row r * G + j
 *   temperature, top_k, top_p  [rows * G]     one entry per logits row, as qqq_sample_tokens takes them
 *   u            f32   [rows, u_stride]       draw j of row r uses u[r, ((unsigned)tick[r] * G + j) % u_stride], tick[r] as before the call
 *   tick         int32 [rows]                 incremented for every row on every call, active or not
 *   ids          int64 [rows, G]              the next forward's input tokens: [r, 0] the last emitted token, [r, 1 ... K] the drafts
 *   pos          int64 [rows, G]              their positions p, p + 1, ... p + K; -1 marks an idle row
 *   slots        int64 [rows, G]              their cache slots, -1 when idle
 *   start        int64 [rows]                 = pos[r, 0], -1 when idle: `start_pos` of qqq_prefill_attn_paged*
 *   block_table  int32 [rows, table_stride]   only read
 *   remaining    int32 [rows]                 tokens the row may still emit; 0 (or less) marks an idle row
 *   eos          int32 [rows]                 per-row eos id, -1 for none; only read
 *   hist         int32 [rows, hist_stride]    the sequence so far, prompt and emitted tokens
 *   hist_len     int32 [rows]                 its length; for an active row hist[r, hist_len - 1] == ids[r, 0], pos[r, 0] == hist_len - 1
 *   n_out        int32 [rows]                 tokens emitted since the host last cleared it: they are hist[r, hist_len - n_out : hist_len]
 *   n_acc        int32 [rows]                 drafts accepted since the host last cleared it (a statistic)
 *   workspace    qqq_spec_advance_workspace_bytes(rows, draft_len) bytes, 8-byte aligned: the draws
 *
 * The draws s_0 ... s_K of row r: s_j is exactly the token qqq_sample_tokens returns for logits row r * G + j, its parameters and the
 * variate above.  Then, for one row:
 *   always                tick[r] += 1
 *   remaining[r] <= 0     nothing else is written
 *   otherwise             rem = remaining[r], p = pos[r, 0], L = hist_len[r]; for j = 0, 1, ...:
 *                           hist[r, L] = s_j; L += 1; n_out[r] += 1; rem -= 1
 *                           stop and retire the row if s_j == eos[r] or rem == 0
 *                           stop if j == K, or if s_j != ids[r, j + 1] (the draft was wrong: the later logits rows saw a false prefix)
 *                           n_acc[r] += 1
 *                         hist_len[r] = L.  With e tokens emitted, p' = p + e is the position of the last one.  The row retires as well
 *                         if L >= hist_stride (no room for another token) or (p' + K) / block_size >= table_stride.  Every index is
 *                         checked before it is used: an append at L == hist_stride is not made and retires the row, and state no caller
 *                         can reach through this entry (hist_len outside [1, hist_stride), pos[r, 0] < 0) retires it with no append.
 *     active              ids[r, 0] = hist[r, L - 1]; ids[r, 1 + j] = d_j; pos[r, j] = p' + j;
 *                         slots[r, j] = block_table[r, (p' + j) / block_size] * block_size + (p' + j) % block_size; start[r] = p';
 *                         remaining[r] = rem
 *     retired             ids[r, :] = 0; pos[r, :] = slots[r, :] = -1; start[r] = -1; remaining[r] = 0   (idle from here on)
 *
 * The drafts d_0 ... d_{K-1} (prompt lookup), from h = hist[r, 0 ... L):
 *   for n = ngram_max down to 1, only while n < L: the largest i < L - n with h[i ... i + n) == h[L - n ... L); the first n that has one wins
 *   d_j = h[i + n + j] if i + n + j < L, else d_{i + n + j - L}   (an overlapping copy: a period continues)
 *   no n matches: d_j = h[L - 1] for every j
 *
 * Why drafting changes no distribution: every emitted token is a plain sampler draw from logits computed on the true prefix.  Rejected
 * drafts leave key / value rows at positions p' + 1 ... p + K; the next call's forward starts at p' and rewrites p' ... p' + K >= p + K
 * before any query attends to them.  An idle row is inert as in include/qqq_amd_step.h: qqq_rope_qkv_paged* writes nothing for
 * position / slot -1 and qqq_prefill_attn_paged* nothing for a sequence with start_pos < 0.
 *
 * Two launches: the sampler's row body over rows * G workgroups (qqq_spec_draw_kernel), then one workgroup per row
 * (qqq_spec_advance_kernel) whose lanes scan hist for the match.  The launch sizes depend on (rows, draft_len, vocab) alone and nothing
 * is read on the host.
 *
 * Conventions are those of include/qqq_amd.h: work only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state.
 * Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error() that begins with the entry's name; bad arguments
 * are rejected before any launch: rows >= 0, 1 <= draft_len <= 15, rows * G <= 65535, 1 <= ngram_max <= 4, the sampler's shape checks
 * (1 <= vocab <= 262144, ld >= vocab, ld % 8 == 0), block_size a power of two in [16, 256], table_stride and hist_stride >= 1,
 * u_stride >= G, every pointer non-NULL, logits 16-byte, the int64 arrays (ids, pos, slots, start) and the workspace 8-byte and
 * everything else 4-byte aligned, workspace_bytes at least what qqq_spec_advance_workspace_bytes returns.  rows == 0 is a no-op (NULL
 * pointers allowed).
 */
#ifndef QQQ_AMD_SPEC_H_
#define QQQ_AMD_SPEC_H_

#include <stddef.h>

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of `workspace` for a call with these rows and draft_len; 0 for arguments the call rejects */
size_t qqq_spec_advance_workspace_bytes(int rows, int draft_len);

int qqq_spec_advance(const void* logits, int ld, const void* temperature, const void* top_k, const void* top_p, const void* u, int u_stride,
                     void* tick, void* ids, void* pos, void* slots, void* start, const void* block_table, int table_stride,
                     void* remaining, const void* eos, void* hist, int hist_stride, void* hist_len, void* n_out, void* n_acc,
                     void* workspace, size_t workspace_bytes, int rows, int draft_len, int ngram_max, int vocab, int block_size, int dev,
                     void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_SPEC_H_ */
