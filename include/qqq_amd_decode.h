/*
 * qqq_amd_decode.h -- C-ABI of the split-K decode attention of a Llama / Qwen2 attention block (exported by libqqq_amd.so, beside
 * include/qqq_amd.h, include/qqq_amd_act.h and include/qqq_amd_attn.h).
 *
 * At decode (one query token per batch row) qqq_decode_attn replaces scaled_dot_product_attention and the dynamic_quant in front of o_proj:
 * it reads the static KV cache that qqq_rope_qkv filled, splits each row's keys over workgroups (flash decoding), takes all query heads
 * of a KV head together (K and V are read once per KV head) and writes o_proj's input already int8-quantised.
 *
 * Conventions are those of include/qqq_amd.h: device pointers on device `dev`, work only ENQUEUED on `stream` (hipStream_t as void*;
 * safe under hipGraph capture), no allocation, no state.  Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in
 * qqq_amd_last_error(); bad arguments are rejected before any launch.  b = 0 is a no-op.
 */
#ifndef QQQ_AMD_DECODE_H_
#define QQQ_AMD_DECODE_H_

#include <stddef.h>

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Attention of one query token per batch row over keys 0 ... pos[bi] of the cache, then the per-token int8 quantisation of the result.
 *   q         fp16 [b, h, 1, d] contiguous (qqq_rope_qkv's q_out at s = 1)
 *   k_cache, v_cache  fp16 [b, kvh, cap, d] contiguous; query head hq reads KV head hq / (h / kvh)
 *   pos       int64 [b], device memory: row bi attends keys 0 ... pos[bi] (qqq_rope_qkv's positions: the new token is already cached)
 *   scale     the score scale (head_dim^-0.5 for Llama / Qwen2)
 *   o_fp16    fp16 [b, h*d] or NULL: the attention output, heads side by side (SDPA's output transposed to [b, 1, h*d])
 *   xq, s1    int8 [b, h*d] and f32 [b, 1], or both NULL: dynamic_quant of the o_fp16 row, bit for bit
 *   workspace at least qqq_decode_attn_workspace_bytes(b, h, kvh, d, max_len) bytes of device memory; contents need no initialisation
 *   max_len   1 <= max_len <= cap: the launch is sized for rows with positions below max_len, read from device memory only at run time,
 *             so a graph captured with max_len = cap replays correctly at every position
 * Arithmetic: scores (q.k) * scale with fp16 inputs, fp32 accumulation and fp32 softmax; the probabilities are rounded to fp16 for the
 * P.V product, accumulated in fp32; the output is rounded to fp16 once.
 * A row whose position is outside [0, min(cap, max_len)) writes nothing: no o_fp16 row, no xq row, no s1.  Nothing outside the given
 * buffers is written; the caches are only read.
 * Shapes: h, kvh >= 1, h % kvh == 0, h / kvh <= 8, d in {64, 128}, h * d <= 16384, b <= 65535.
 * Alignment: q, the caches, o_fp16 and workspace 16 bytes; pos and xq 8 bytes; s1 4 bytes.
 */
int qqq_decode_attn(const void* q, const void* k_cache, const void* v_cache, const void* pos, float scale, void* o_fp16, void* xq, void* s1,
                    void* workspace, size_t workspace_bytes, int b, int h, int kvh, int d, int cap, int max_len, int dev, void* stream);

/* Bytes of workspace qqq_decode_attn needs for these sizes (non-decreasing in max_len); 0 for b = 0 or sizes it would reject. */
size_t qqq_decode_attn_workspace_bytes(int b, int h, int kvh, int d, int max_len);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_DECODE_H_ */
