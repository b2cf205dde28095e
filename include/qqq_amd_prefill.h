/*
 * qqq_amd_prefill.h -- C-ABI of the paged prefill attention of a Llama / Qwen2 attention block (exported by libqqq_amd.so, beside
 * include/qqq_amd.h, include/qqq_amd_act.h, include/qqq_amd_attn.h, include/qqq_amd_decode.h, include/qqq_amd_kv8.h and
 * include/qqq_amd_paged.h).
 *
 * One call serves a packed batch of b sequences that bring any number of tokens each -- prompt prefill, chunked prefill, chunks batched
 * with decoding rows -- over the block pools of include/qqq_amd_paged.h, read in place through the block table:
 *   q            fp16 [m, h, d] token-major: qqq_rope_qkv_paged's q_out.  The call's new tokens are already in the pool, as for decode.
 *   k_pool, v_pool, k_scale, v_scale, block_table (int32 [b, table_stride])   as in include/qqq_amd_paged.h
 *   cu_tokens    int32 [b + 1] in device memory: cu_tokens[0] = 0, non-decreasing, cu_tokens[b] <= m
 *   start_pos    int64 [b] in device memory
 * Token t with cu_tokens[i] <= t < cu_tokens[i + 1] belongs to sequence i, sits at position start_pos[i] + t - cu_tokens[i] and attends
 * keys 0 ... that position of row i of the block table (causal inside the chunk).
 *
 * Arithmetic: qqq_decode_attn's -- fp16 inputs, fp32 score accumulation, fp32 online softmax in the log2 domain over 32-key steps aligned
 * to the absolute key index, probabilities rounded to fp16 for P V, accumulated in fp32, the output rounded to fp16 once.  An int8 pool
 * follows qqq_decode_attn_kv8: scores from the codes times the key's scale, V as fp16(float(code) * scale).  There is no split over keys:
 * an output row is a function of its own query, position and keys only, whatever else the call holds.
 *   o_fp16   fp16 [m, h*d] or NULL;   xq int8 [m, h*d] and s1 f32 [m, 1], both or neither: bit for bit qqq_dynamic_quant of the fp16 row
 *   workspace    qqq_prefill_attn_workspace_bytes(m, h, d) bytes, needed where o_fp16 is NULL (the fp16 rows live there)
 * Two launches: the attention, and the quantisation of the rows it wrote (only where xq / s1 are given).
 *
 * Only table entries 0 ... (start_pos[i] + count_i - 1) / block_size of row i are read, and no key beyond a sequence's last one: the rest
 * of the table and of the pool may hold anything.  A block id that is read is clamped into [0, num_blocks).  A sequence with start_pos[i]
 * < 0 or start_pos[i] + count_i > max_len writes nothing; tokens >= cu_tokens[b] are padding and write nothing; unwritten rows are left
 * untouched in o_fp16, xq and s1.  The pools are only read.  The launch sizes depend on (m, b, h, kvh, d) alone: a captured graph replays
 * with other contents of cu_tokens, start_pos, block_table and the pools.
 *
 * Conventions are those of include/qqq_amd.h: work only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state.
 * Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error() that begins with the entry's name; bad arguments
 * are rejected before any launch.  m = 0 and b = 0 are no-ops (NULL pointers allowed).
 * Shapes: h % kvh == 0, h / kvh <= 8, d in {64, 128}, h*d <= 16384, b <= 65535, block_size a power of two in [16, 256], num_blocks >= 1,
 * num_blocks * block_size < 2^31, table_stride >= 1, 1 <= max_len <= table_stride * block_size.
 * Alignment: q, the pools, o_fp16 and workspace 16 bytes; start_pos and xq 8 bytes; cu_tokens, block_table, the scales and s1 4 bytes.
 */
#ifndef QQQ_AMD_PREFILL_H_
#define QQQ_AMD_PREFILL_H_

#include <stddef.h>

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of workspace a call with o_fp16 == NULL needs: the fp16 rows [m, h*d]; 0 for m == 0 or a shape the entries reject */
size_t qqq_prefill_attn_workspace_bytes(int m, int h, int d);

int qqq_prefill_attn_paged(const void* q, const void* k_pool, const void* v_pool, const void* block_table, int table_stride,
                           const void* cu_tokens, const void* start_pos, float scale, void* o_fp16, void* xq, void* s1, void* workspace,
                           size_t workspace_bytes, int m, int b, int h, int kvh, int d, int num_blocks, int block_size, int max_len, int dev,
                           void* stream);

/* the same over an int8 pool with its scales */
int qqq_prefill_attn_paged_kv8(const void* q, const void* k_pool, const void* v_pool, const void* k_scale, const void* v_scale,
                               const void* block_table, int table_stride, const void* cu_tokens, const void* start_pos, float scale,
                               void* o_fp16, void* xq, void* s1, void* workspace, size_t workspace_bytes, int m, int b, int h, int kvh,
                               int d, int num_blocks, int block_size, int max_len, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_PREFILL_H_ */
