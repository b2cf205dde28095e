/*
 * qqq_amd_attn.h -- C-ABI of the rotary embedding + KV-cache write of a Llama / Qwen2 attention block (exported by libqqq_amd.so, beside
 * include/qqq_amd.h and include/qqq_amd_act.h).
 *
 * Between the q/k/v projections and the attention core, transformers' eager path launches ~10 small kernels for RoPE, concatenates the
 * new k/v onto the cache history and makes q contiguous.  qqq_rope_qkv does all of it in ONE launch: it reads each token's q, k and v rows
 * straight from the projection output, rotates q and k, writes q in scaled_dot_product_attention's layout and writes rotated k and plain v
 * into a static cache at the token's position.
 *
 * Conventions are those of include/qqq_amd.h: device pointers on device `dev`, work only ENQUEUED on `stream` (hipStream_t as void*;
 * safe under hipGraph capture), no allocation, no state.  Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in
 * qqq_amd_last_error(); bad arguments are rejected before any launch.  b = 0 or s = 0 (no tokens) is a no-op.
 */
#ifndef QQQ_AMD_ATTN_H_
#define QQQ_AMD_ATTN_H_

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * RoPE on q and k, q to SDPA layout, k and v into the cache.  m = b * s tokens, token t = bi * s + si.
 *   q, k, v   fp16, m rows of h*d, kvh*d, kvh*d elements with row strides ld_q, ld_k, ld_v (elements, multiples of 8, >= the row width)
 *             -- e.g. the three column ranges of one fused q|k|v GEMM output [m, (h + 2 kvh) d], read in place
 *   cos, sin  fp16 [table_len, d], row p = the table at position p (built by the host; the kernel evaluates no transcendental)
 *   pos       int64 [m], device memory: the position of token t
 *   q_out     fp16 [b, h, s, d] contiguous
 *   k_cache, v_cache  fp16 [b, kvh, cap, d] contiguous: token (bi, si) goes to slot pos[t] of batch row bi
 * Arithmetic: transformers' apply_rotary_pos_emb on fp16, with rotate_half(x) = cat(-x[d/2:], x[:d/2]):
 *   out = fp16(fp16(x * cos[p]) + fp16(rotate_half(x) * sin[p])) per element (no fused multiply-add); v is copied bit for bit.
 * A token whose position is outside [0, min(cap, table_len)) writes nothing: no q_out row, no cache slot (its q_out row keeps whatever it
 * held).  Nothing outside the given buffers is written.  q_out and the caches must not overlap q / k / v / cos / sin / pos.
 * Shapes: h, kvh >= 1, h % kvh == 0, d a multiple of 16 in [16, 256], (h + 2 kvh) * d <= 1 << 20, cap >= 0, table_len >= 0.
 * Alignment: every fp16 pointer 16 bytes, pos 8 bytes.
 */
int qqq_rope_qkv(const void* q, int ld_q, const void* k, int ld_k, const void* v, int ld_v, const void* cos, const void* sin,
                 int table_len, const void* pos, void* q_out, void* k_cache, void* v_cache, int b, int s, int h, int kvh, int d, int cap,
                 int dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_ATTN_H_ */
