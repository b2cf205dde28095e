/*
 * qqq_amd_step.h -- C-ABI of the decode loop's sample-and-advance step (exported by libqqq_amd.so, beside include/qqq_amd.h and the other
 * per-feature headers): qqq_sample_tokens (include/qqq_amd_sample.h) with an epilogue that does, on the device, everything a decode loop
 * does between two steps -- record the token, check eos and budget, move the row to its next position and cache slot, or retire it.  With
 * it a whole decode step (model forward + this call) reads nothing on the host and can be captured into ONE graph that is replayed many
 * times between host syncs, while rows finish and join without re-capture.
 *
 * Per-row state of `rows` rows, all in device memory:
 *   logits, ld, temperature, top_k, top_p   as qqq_sample_tokens, unchanged semantics
 *   u            f32   [rows, u_stride]       row r draws with u[r, tick[r] % u_stride] (tick taken as unsigned)
 *   tick         int32 [rows]                 incremented for every row on every call, active or not
 *   ids          int64 [rows]                 the row's next input token: the embedding index of the next step
 *   pos          int64 [rows]                 position of the token in ids -- `pos` of qqq_rope_qkv_paged* and `pos` (the last position)
 *                                             of qqq_decode_attn_paged* alike; -1 marks an idle row
 *   slots        int64 [rows]                 cache slot of that token, -1 when idle
 *   block_table  int32 [rows, table_stride]   only read
 *   remaining    int32 [rows]                 tokens the row may still emit; 0 (or less) marks an idle row
 *   eos          int32 [rows]                 per-row eos id, -1 for none; only read
 *   out          int64 [rows, out_stride]     emitted tokens
 *   n_out        int32 [rows]                 number of tokens written to out[r]
 *
 * One row r, by one lane after the draw (t is exactly the token qqq_sample_tokens returns for the same logits, parameters and variate):
 *   always                tick[r] += 1
 *   remaining[r] <= 0     nothing else is written
 *   otherwise             out[r, n_out[r]] = t;  n_out[r] += 1;  rem = remaining[r] - 1;  rem = 0 if t == eos[r]
 *                         p = pos[r] + 1;  rem = 0 as well if p / block_size >= table_stride or n_out[r] >= out_stride, so a corrupt budget
 *                         never indexes outside the table or out.  (State no caller can reach through this entry is treated alike: an
 *                         n_out[r] outside [0, out_stride) writes no token and retires the row, and so does p < 0.)
 *     rem > 0             ids[r] = t;  pos[r] = p;  slots[r] = block_table[r, p / block_size] * block_size + p % block_size;
 *                         remaining[r] = rem
 *     rem == 0            ids[r] = 0;  pos[r] = -1;  slots[r] = -1;  remaining[r] = 0      (the row is idle from here on)
 *
 * An idle row rides along in every later step and is inert: qqq_rope_qkv_paged* writes nothing for a position outside its table (pos -1)
 * and no cache row for slot -1; qqq_decode_attn_paged* writes nothing for a position outside [0, max_len); every other op of a decode step
 * (embedding, norms, GEMMs, activation, the sampler) is row-wise.  So whatever bits an idle row carries -- its activations are whatever the
 * skipped writes left in memory -- they never reach an active row, the KV pool, or (remaining being 0) out.
 *
 * One launch, one workgroup per row; the launch size depends on (rows, vocab) alone and nothing is read on the host.  No workspace.
 *
 * Conventions are those of include/qqq_amd.h: work only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state.
 * Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error() that begins with the entry's name; bad arguments
 * are rejected before any launch: the sampler's own checks (1 <= vocab <= 262144, ld >= vocab, ld % 8 == 0, 0 <= rows <= 65535),
 * block_size a power of two in [16, 256], table_stride, out_stride, u_stride >= 1, every pointer non-NULL, logits 16-byte, the int64 arrays
 * (ids, pos, slots, out) 8-byte and everything else 4-byte aligned.  rows == 0 is a no-op (NULL pointers allowed).
 */
#ifndef QQQ_AMD_STEP_H_
#define QQQ_AMD_STEP_H_

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int qqq_sample_advance(const void* logits, int ld, const void* temperature, const void* top_k, const void* top_p, const void* u,
                       int u_stride, void* tick, void* ids, void* pos, void* slots, const void* block_table, int table_stride,
                       void* remaining, const void* eos, void* out, int out_stride, void* n_out, int rows, int vocab, int block_size,
                       int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_STEP_H_ */
