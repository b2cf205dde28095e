/*
 * qqq_amd_kv8.h -- C-ABI of the int8 KV cache of a Llama / Qwen2 attention block (exported by libqqq_amd.so, beside include/qqq_amd.h,
 * include/qqq_amd_act.h, include/qqq_amd_attn.h and include/qqq_amd_decode.h).
 *
 * The cache holds every head row (one token, one KV head, d elements) as dynamic_quant of the fp16 row the fp16 cache would hold
 * (include/qqq_amd_act.h: s = float(fp16(amax / 127)), code = clamp(rint(y / s), -128, 127), an all-zero row gives zero codes):
 *   k_cache, v_cache  int8 [b, kvh, cap, d] contiguous
 *   k_scale, v_scale  f32  [b, kvh, cap]    contiguous
 * d + 4 bytes per row against 2 d.  The rope / cache-write variant quantises the rows as it stores them, the decode-attention variant
 * reads them; both keep the semantics of their fp16 counterparts in include/qqq_amd_attn.h and include/qqq_amd_decode.h.
 *
 * Conventions are those of include/qqq_amd.h: device pointers on device `dev`, work only ENQUEUED on `stream` (hipStream_t as void*;
 * safe under hipGraph capture), no allocation, no state.  Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in
 * qqq_amd_last_error(); bad arguments are rejected before any launch.  b = 0 (and s = 0) is a no-op.
 */
#ifndef QQQ_AMD_KV8_H_
#define QQQ_AMD_KV8_H_

#include <stddef.h>

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * qqq_rope_qkv with an int8 cache, one launch.  q, k, v, cos, sin, pos, q_out and the sizes are qqq_rope_qkv's; q_out is bit for bit
 * qqq_rope_qkv's.  The rotated k row and the plain v row of token (bi, si) and KV head hk go to slot pos[bi*s + si] of row (bi, hk) as d
 * codes in k_cache / v_cache and one scale in k_scale / v_scale: bit for bit dynamic_quant of the fp16 row qqq_rope_qkv would have cached.
 * A token whose position is outside [0, min(cap, table_len)) writes nothing: no codes, no scale, no q_out row.
 * Shapes: qqq_rope_qkv's, with d in {64, 128}.  Alignment: fp16 tensors and the caches 16 bytes, pos 8 bytes, the scales 4 bytes.
 */
int qqq_rope_qkv_kv8(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* cos, const void* sin,
                     int table_len, const void* pos, void* q_out, void* k_cache, void* v_cache, void* k_scale, void* v_scale, int b, int s,
                     int h, int kvh, int d, int cap, int dev, void* stream);

/*
 * qqq_decode_attn over an int8 cache: two launches, the second one qqq_decode_attn's combine.  q, pos, scale, o_fp16, xq, s1, workspace
 * (qqq_decode_attn_workspace_bytes), max_len, the shape limits and the out-of-range rule are qqq_decode_attn's; the caches are only read.
 * Arithmetic: q stays fp16; the codes enter as exact fp16 numbers; a score is (q . code_k), accumulated in fp32, times
 * k_scale[key] * scale in fp32; fp32 softmax; the probabilities are rounded to fp16; a value enters the P.V product as
 * fp16(code_v * v_scale[key]), the product computed in fp32; fp32 accumulation; the output is rounded to fp16 once and (xq, s1) is
 * dynamic_quant of that row, bit for bit.
 * Alignment: q, the caches, o_fp16 and workspace 16 bytes; pos and xq 8 bytes; s1 and the scales 4 bytes.
 */
int qqq_decode_attn_kv8(const void* q, const void* k_cache, const void* v_cache, const void* k_scale, const void* v_scale, const void* pos,
                        float scale, void* o_fp16, void* xq, void* s1, void* workspace, size_t workspace_bytes, int b, int h, int kvh, int d,
                        int cap, int max_len, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_KV8_H_ */
