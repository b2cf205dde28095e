/*
 * qqq_amd_paged.h -- C-ABI of the block-table (paged) KV cache of a Llama / Qwen2 attention block (exported by libqqq_amd.so, beside
 * include/qqq_amd.h, include/qqq_amd_act.h, include/qqq_amd_attn.h, include/qqq_amd_decode.h and include/qqq_amd_kv8.h).
 *
 * The cache of one layer is a pool of blocks of block_size keys that any sequence may own:
 *   k_pool, v_pool    fp16 or int8 [num_blocks, kvh, block_size, d] contiguous
 *   k_scale, v_scale  f32 [num_blocks, kvh, block_size] contiguous (int8 pools only: every head row is dynamic_quant of the fp16 row, as
 *                     in include/qqq_amd_kv8.h)
 * block_size is a power of two in [16, 256], d is 64 or 128.  A token's row lives at slot = block * block_size + offset; a sequence's keys
 * are found through its row of a block table (key j in block block_table[row][j / block_size] at offset j % block_size).  Sequences of
 * different lengths share one call, finished sequences' blocks are reused, several rows may name the same blocks (a common prefix).
 * The entry points keep the arithmetic of their contiguous counterparts bit for bit; only the addresses differ.
 *
 * Conventions are those of include/qqq_amd.h: device pointers on device `dev`, work only ENQUEUED on `stream` (hipStream_t as void*;
 * safe under hipGraph capture), no allocation, no state.  Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in
 * qqq_amd_last_error(); bad arguments are rejected before any launch.  m = 0 and b = 0 are no-ops.
 */
#ifndef QQQ_AMD_PAGED_H_
#define QQQ_AMD_PAGED_H_

#include <stddef.h>

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * qqq_rope_qkv into an fp16 pool, one launch for the m tokens of the call.  q, k, v (fp16 token rows with row strides ld_q, ld_k, ld_v),
 * cos, sin (fp16 [table_len, d]) and pos (int64 [m], a position per token) are qqq_rope_qkv's.
 *   slots   int64 [m]: token t's rotated k row and plain v row of KV head hk go to row (slots[t] / block_size, hk, slots[t] % block_size)
 *   q_out   fp16 [m, h, d], token-major: the rotated q (for a decode batch, m = b, the memory of [b, h, 1, d])
 * q_out and the cached rows are bit for bit what qqq_rope_qkv produces for the same token and position.
 * A token whose position is outside [0, table_len) writes nothing.  A token whose slot is outside [0, num_blocks * block_size) -- a
 * serving stack's padding slot -1 -- writes its q_out row and no cache row.  Two tokens of one call with the same slot: unspecified.
 * Shapes: m >= 0, h % kvh == 0, d in {64, 128}, (h + 2 kvh) d <= 2^20, num_blocks >= 1, num_blocks * block_size < 2^31, row strides
 * multiples of 8 and >= h*d / kvh*d.  Alignment: fp16 tensors and the pools 16 bytes, pos and slots 8 bytes.
 */
int qqq_rope_qkv_paged(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* cos, const void* sin,
                       int table_len, const void* pos, const void* slots, void* q_out, void* k_pool, void* v_pool, int m, int h, int kvh,
                       int d, int num_blocks, int block_size, int dev, void* stream);

/*
 * The same into an int8 pool: every cached row is stored as d codes and one scale, bit for bit what qqq_rope_qkv_kv8 stores for the same
 * token and position; q_out is qqq_rope_qkv_paged's.  Alignment: as above, the scales 4 bytes.
 */
int qqq_rope_qkv_paged_kv8(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* cos, const void* sin,
                           int table_len, const void* pos, const void* slots, void* q_out, void* k_pool, void* v_pool, void* k_scale,
                           void* v_scale, int m, int h, int kvh, int d, int num_blocks, int block_size, int dev, void* stream);

/*
 * qqq_decode_attn over an fp16 pool: two launches, the second one qqq_decode_attn's combine.  q (fp16 [b, h, d]), pos (int64 [b]), scale,
 * o_fp16, xq, s1, workspace (qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len)) and the shape limits (h % kvh == 0, h / kvh <= 8,
 * d in {64, 128}, h*d <= 16384, b <= 65535) are qqq_decode_attn's.
 *   block_table   int32 [b, table_stride] in device memory, table_stride >= 1;  1 <= max_len <= table_stride * block_size
 * Row bi attends keys 0 ... pos[bi]; a row with pos[bi] outside [0, max_len) writes nothing.  Only table entries 0 ... pos[bi] / block_size
 * of a row are read, the rest may hold anything.  Several rows may name the same block; the pools are only read.  A block id that is read
 * is clamped into [0, num_blocks): a corrupt table gives an unspecified row, never an access outside the pools.
 * The split plan and the order of every sum are qqq_decode_attn's, so for equal (b, kvh, max_len) the outputs o_fp16, xq and s1 are bit
 * for bit those of qqq_decode_attn over a contiguous cache that holds the same rows.
 * Alignment: q, the pools, o_fp16 and workspace 16 bytes; pos and xq 8 bytes; block_table and s1 4 bytes.
 */
int qqq_decode_attn_paged(const void* q, const void* k_pool, const void* v_pool, const void* block_table, int table_stride, const void* pos,
                          float scale, void* o_fp16, void* xq, void* s1, void* workspace, size_t workspace_bytes, int b, int h, int kvh,
                          int d, int num_blocks, int block_size, int max_len, int dev, void* stream);

/*
 * The same over an int8 pool with the arithmetic of qqq_decode_attn_kv8, bit for bit.  Alignment: as above, the scales 4 bytes.
 */
int qqq_decode_attn_paged_kv8(const void* q, const void* k_pool, const void* v_pool, const void* k_scale, const void* v_scale,
                              const void* block_table, int table_stride, const void* pos, float scale, void* o_fp16, void* xq, void* s1,
                              void* workspace, size_t workspace_bytes, int b, int h, int kvh, int d, int num_blocks, int block_size,
                              int max_len, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_PAGED_H_ */
