/*
 * qqq_amd_window.h -- C-ABI of sliding-window attention over the block pools (exported by libqqq_amd.so, beside include/qqq_amd.h,
 * include/qqq_amd_paged.h and include/qqq_amd_prefill.h): the windowed twins of qqq_decode_attn_paged(_kv8) and
 * qqq_prefill_attn_paged(_kv8), for the layers of Mistral, Mixtral and the window layers of Qwen2 / Qwen3.
 *
 * A layer with window W >= 1: the query at position i attends key j iff i - W < j <= i -- W keys, its own included (transformers'
 * sliding_window_overlay: kv_idx > q_idx - sliding_window).  lo(i) = max(0, i - W + 1).
 *   decode    row bi attends keys lo(pos[bi]) ... pos[bi]
 *   prefill   a token at position p attends keys lo(p) ... p
 * Every argument but `window` is that of the unwindowed entry (include/qqq_amd_paged.h, include/qqq_amd_prefill.h), with its shape
 * limits and alignments; window < 1 is QQQ_ERR_ARG.  The arithmetic is the unwindowed entries': fp16 inputs, fp32 scores in the log2
 * domain, online softmax over 32-key steps aligned to the absolute key index, P rounded to fp16, fp32 P V; xq / s1 are bit for bit
 * qqq_dynamic_quant of the fp16 row.
 *
 * What is read.  Only these block-table entries: decode, lo(pos[bi]) / block_size ... pos[bi] / block_size of row bi; prefill, from
 * lo(start_pos[i]) / block_size to (start_pos[i] + count_i - 1) / block_size of row i.  No key below lo of the earliest query a workgroup
 * serves is loaded (decode: the row's; prefill: the first token's of a query tile of 128 / (h / kvh) tokens), nor its scale: entries and
 * pool rows behind the window may hold anything -- NaN, ids of blocks that were freed and serve another sequence.  A block id that is read
 * is clamped into [0, num_blocks).  Rows that write nothing are the unwindowed entries' (pos outside [0, max_len), padding tokens,
 * sequences that do not fit).
 *
 * window >= max_len: every output (o_fp16, xq, s1) is bit for bit the unwindowed entry's for the same call.
 *
 * Decode splits keys over span = min(max_len, round_up(window + 127, 128)), not over max_len: the grid, the workspace and the partials
 * the combine merges follow W.  Each row places the splits at its own window (from lo rounded down to 128), so the launch sizes depend on
 * (b, h, kvh, d, min(max_len, window)) alone; a prefill call's on (m, b, h, kvh, d).  Neither depends on contents: a captured graph
 * replays at other positions, tables and pools.
 *   workspace   decode: qqq_decode_attn_window_workspace_bytes(b, h, kvh, d, max_len, window) bytes;
 *               prefill: qqq_prefill_attn_workspace_bytes(m, h, d), where o_fp16 is NULL
 *
 * Conventions are those of include/qqq_amd.h: work only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state.
 * Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error() that begins with the entry's name; bad arguments
 * are rejected before any launch.  b = 0 and m = 0 are no-ops (NULL pointers allowed).
 */
#ifndef QQQ_AMD_WINDOW_H_
#define QQQ_AMD_WINDOW_H_

#include <stddef.h>

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of workspace of a windowed decode call; 0 for b == 0, window < 1 or a shape the entries reject */
size_t qqq_decode_attn_window_workspace_bytes(int b, int h, int kvh, int d, int max_len, int window);

int qqq_decode_attn_paged_window(const void* q, const void* k_pool, const void* v_pool, const void* block_table, int table_stride,
                                 const void* pos, float scale, void* o_fp16, void* xq, void* s1, void* workspace, size_t workspace_bytes,
                                 int b, int h, int kvh, int d, int num_blocks, int block_size, int max_len, int window, int dev,
                                 void* stream);

/* the same over an int8 pool with its scales */
int qqq_decode_attn_paged_window_kv8(const void* q, const void* k_pool, const void* v_pool, const void* k_scale, const void* v_scale,
                                     const void* block_table, int table_stride, const void* pos, float scale, void* o_fp16, void* xq,
                                     void* s1, void* workspace, size_t workspace_bytes, int b, int h, int kvh, int d, int num_blocks,
                                     int block_size, int max_len, int window, int dev, void* stream);

int qqq_prefill_attn_paged_window(const void* q, const void* k_pool, const void* v_pool, const void* block_table, int table_stride,
                                  const void* cu_tokens, const void* start_pos, float scale, void* o_fp16, void* xq, void* s1,
                                  void* workspace, size_t workspace_bytes, int m, int b, int h, int kvh, int d, int num_blocks,
                                  int block_size, int max_len, int window, int dev, void* stream);

/* the same over an int8 pool with its scales */
int qqq_prefill_attn_paged_window_kv8(const void* q, const void* k_pool, const void* v_pool, const void* k_scale, const void* v_scale,
                                      const void* block_table, int table_stride, const void* cu_tokens, const void* start_pos,
                                      float scale, void* o_fp16, void* xq, void* s1, void* workspace, size_t workspace_bytes, int m,
                                      int b, int h, int kvh, int d, int num_blocks, int block_size, int max_len, int window, int dev,
                                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_WINDOW_H_ */
