/*
 * qqq_amd_verify.h -- C-ABI of the attention of a verify chunk over the block-table (paged) KV cache: t consecutive tokens per batch row,
 * as the step of a speculative decode loop feeds them (exported by libqqq_amd.so, beside include/qqq_amd_paged.h, whose pools, block
 * tables and conventions these entry points share).
 *
 * A chunk's queries ride in the padding of qqq_decode_attn_paged's MFMA operands: K and V are read once per KV head for all t tokens, and
 * the keys stay split over workgroups as for one token.  Every token's outputs are bit for bit those of qqq_decode_attn_paged(_kv8)
 * called for that token alone -- the same b, kvh and max_len, q the token's rows and pos = start + j -- for finite cache rows; at t = 1
 * the call is that call.
 *
 * Conventions are those of include/qqq_amd.h: device pointers on device `dev`, work only ENQUEUED on `stream` (hipStream_t as void*;
 * safe under hipGraph capture), no allocation, no state.  Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in
 * qqq_amd_last_error(); bad arguments are rejected before any launch.  b = 0 is a no-op.  The launch sizes depend on (b, t, h, kvh,
 * max_len) alone, so a captured graph replays with other contents of every tensor.
 */
#ifndef QQQ_AMD_VERIFY_H_
#define QQQ_AMD_VERIFY_H_

#include <stddef.h>

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Two launches over an fp16 pool.
 *   q             fp16 [b * t, h, d], token-major: qqq_rope_qkv_paged's q_out of the chunk (token j of row r is row r * t + j)
 *   k_pool, v_pool, block_table, table_stride, num_blocks, block_size   as for qqq_decode_attn_paged; the chunk's own keys are in the pool
 *   start         int64 [b] in device memory: the position of row r's first token; token j attends keys 0 ... start[r] + j
 *   o_fp16, xq, s1   fp16 [b * t, h*d] or NULL, int8 [b * t, h*d] and f32 [b * t, 1] (both or neither)
 *   workspace     qqq_verify_attn_workspace_bytes(b, t, h, kvh, d, max_len) bytes
 * Token j of row r writes nothing (no fp16 row, no xq, no s1) if start[r] < 0 or start[r] + j >= max_len; the row's other tokens are not
 * affected.  Only table entries 0 ... (start[r] + t - 1) / block_size of a row are read; block ids are clamped into [0, num_blocks).
 * Shapes: the limits of qqq_decode_attn_paged (h % kvh == 0, h / kvh <= 8, d in {64, 128}, h*d <= 16384), 1 <= t <= 16,
 * (h / kvh) * t <= 64, b * t <= 65535, 1 <= max_len <= table_stride * block_size.  Alignment: q, the pools, o_fp16 and workspace 16
 * bytes, start and xq 8 bytes, block_table and s1 4 bytes.
 */
int qqq_verify_attn_paged(const void* q, const void* k_pool, const void* v_pool, const void* block_table, int table_stride,
                          const void* start, float scale, void* o_fp16, void* xq, void* s1, void* workspace, size_t workspace_bytes,
                          int b, int t, int h, int kvh, int d, int num_blocks, int block_size, int max_len, int dev, void* stream);

/*
 * The same over an int8 pool (k_scale, v_scale f32 [num_blocks, kvh, block_size], 4-byte aligned), with qqq_decode_attn_paged_kv8's
 * arithmetic.
 */
int qqq_verify_attn_paged_kv8(const void* q, const void* k_pool, const void* v_pool, const void* k_scale, const void* v_scale,
                              const void* block_table, int table_stride, const void* start, float scale, void* o_fp16, void* xq,
                              void* s1, void* workspace, size_t workspace_bytes, int b, int t, int h, int kvh, int d, int num_blocks,
                              int block_size, int max_len, int dev, void* stream);

/* qqq_decode_attn_workspace_bytes(b * t, h, kvh, d, max_len); 0 for b = 0 or a shape the entry points refuse */
size_t qqq_verify_attn_workspace_bytes(int b, int t, int h, int kvh, int d, int max_len);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_VERIFY_H_ */
