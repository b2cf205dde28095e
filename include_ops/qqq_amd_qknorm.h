/*
 * qqq_amd_qknorm.h -- C-ABI of the per-head q / k RMSNorm fused into the rotary embedding + KV-cache write of a Qwen3 attention block
 * (exported by libqqq_amd.so, beside include/qqq_amd.h, include/qqq_amd_attn.h, include/qqq_amd_kv8.h and include/qqq_amd_paged.h).
 *
 * Qwen3 puts an RMSNorm over head_dim (q_norm, k_norm: weight [d], eps = rms_norm_eps) between the q / k projections and RoPE.  The four
 * entry points below are qqq_rope_qkv, qqq_rope_qkv_kv8, qqq_rope_qkv_paged and qqq_rope_qkv_paged_kv8 with that norm in front of the
 * rotation, still ONE launch: each takes its counterpart's argument list with q_weight, k_weight and eps inserted after ld_v, and keeps
 * its counterpart's layouts, position / slot rules, limits and alignment.  Only d in {64, 128} is taken (all four).
 *   q_weight, k_weight   fp16 [d], 16-byte aligned: the weights of q_norm and k_norm
 *   eps                  >= 0, finite
 *
 * Arithmetic of a q or k head row x (fp16, d elements) with weight w -- transformers' Qwen3RMSNorm on an fp16 tensor, with the mean
 * taken in a stated order and in f64:
 *   ss    = sum of double(x[e])^2 in f64 (every square is exact), in this order: the row is spread over P = d / 16 neighbouring lanes,
 *           lane i of a head holding elements 8i .. 8i+7 (low) and d/2 + 8i .. d/2 + 8i+7 (high); a lane adds its 8 low squares, then its
 *           8 high squares, ascending, onto 0.0; then an xor butterfly over the lanes: ss += ss of lane ^ 1, then of lane ^ 2, then
 *           (P = 8) of lane ^ 4.  Every lane of a head ends with the same bits.
 *   var   = float(ss / d)                              (d is a power of two: exact in f64, one rounding to f32)
 *   rs    = 1.0f / sqrtf(var + eps)                    (f32 add, f32 square root and f32 reciprocal, each correctly rounded)
 *   n[e]  = fp16(float(x[e]) * rs)
 *   y[e]  = fp16(float(w[e]) * float(n[e]))
 * y then goes through the rotation exactly as x does in qqq_rope_qkv (include/qqq_amd_attn.h: two rounded products, one rounded add, no
 * fused multiply-add), and an int8 cache stores dynamic_quant of the rotated row as in include/qqq_amd_kv8.h.  v rows are untouched.  So
 * with y in place of x, q_out and every cached row, code and scale are bit for bit the counterpart's.  An all-zero row gives zeros.
 *
 * Conventions are those of include/qqq_amd.h: device pointers on device `dev`, work only ENQUEUED on `stream` (hipStream_t as void*;
 * safe under hipGraph capture), no allocation, no state.  Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in
 * qqq_amd_last_error(); bad arguments are rejected before any launch.  No tokens (b = 0, s = 0, m = 0) is a no-op.
 */
#ifndef QQQ_AMD_QKNORM_H_
#define QQQ_AMD_QKNORM_H_

#include <stddef.h>

#include "../include/qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * qqq_rope_qkv (include/qqq_amd_attn.h) with the norm: q_out fp16 [b, h, s, d], k_cache / v_cache fp16 [b, kvh, cap, d].  A token whose
 * position is outside [0, min(cap, table_len)) writes nothing.
 */
int qqq_rope_qkv_norm(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* q_weight, const void* k_weight,
                      float eps, const void* cos, const void* sin, int table_len, const void* pos, void* q_out, void* k_cache,
                      void* v_cache, int b, int s, int h, int kvh, int d, int cap, int dev, void* stream);

/*
 * qqq_rope_qkv_kv8 (include/qqq_amd_kv8.h) with the norm: int8 caches [b, kvh, cap, d] with f32 scales [b, kvh, cap]; every cached row is
 * dynamic_quant of the fp16 row qqq_rope_qkv_norm would have cached, q_out is qqq_rope_qkv_norm's.
 */
int qqq_rope_qkv_norm_kv8(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* q_weight,
                          const void* k_weight, float eps, const void* cos, const void* sin, int table_len, const void* pos, void* q_out,
                          void* k_cache, void* v_cache, void* k_scale, void* v_scale, int b, int s, int h, int kvh, int d, int cap, int dev,
                          void* stream);

/*
 * qqq_rope_qkv_paged (include/qqq_amd_paged.h) with the norm: q_out fp16 [m, h, d] token-major, fp16 pools
 * [num_blocks, kvh, block_size, d].  A token whose position is outside [0, table_len) writes nothing; a token whose slot is outside
 * [0, num_blocks * block_size) writes its q_out row and no cache row.
 */
int qqq_rope_qkv_norm_paged(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* q_weight,
                            const void* k_weight, float eps, const void* cos, const void* sin, int table_len, const void* pos,
                            const void* slots, void* q_out, void* k_pool, void* v_pool, int m, int h, int kvh, int d, int num_blocks,
                            int block_size, int dev, void* stream);

/*
 * qqq_rope_qkv_paged_kv8 with the norm: int8 pools with f32 scales [num_blocks, kvh, block_size]; rows as qqq_rope_qkv_norm_kv8 stores
 * them, q_out and the position / slot rules qqq_rope_qkv_norm_paged's.
 */
int qqq_rope_qkv_norm_paged_kv8(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* q_weight,
                                const void* k_weight, float eps, const void* cos, const void* sin, int table_len, const void* pos,
                                const void* slots, void* q_out, void* k_pool, void* v_pool, void* k_scale, void* v_scale, int m, int h,
                                int kvh, int d, int num_blocks, int block_size, int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_QKNORM_H_ */
