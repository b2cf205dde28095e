// qqq_attn.hip.h -- the rotary embedding and KV-cache write of a Llama / Qwen2 attention block (include/qqq_amd_attn.h).  Part of the single
// translation unit qqq_w4a8.hip.
//
// One launch per layer and step: each token's q, k and v rows are read straight from the projection output (three views into one fused
// q|k|v GEMM output, or three tensors), q and k are rotated, q is written in SDPA layout [b, h, s, d] and rotated k / plain v go into the
// static cache [b, kvh, cap, d] at the token's position, read from device memory (pos), so a captured graph replays with new positions.
//
// Decomposition: a work item is one 16-byte vector of the first half of a head paired with the matching vector of the second half
// (P = d / 16 items per head), for the h q heads, then the kvh k heads, then the kvh v heads.  Grid x = token, grid y = blocks of NT items,
// one item per lane; no LDS, no loop, no cross-lane traffic.  A token whose position is outside [0, limit) returns before any load.
//
// Arithmetic: transformers' apply_rotary_pos_emb on fp16 tensors, which torch evaluates per element in fp32 and rounds to fp16 after each op:
//   out[e]       = fp16(fp16(x[e] * cos[e])       + fp16(-x[e + d/2] * sin[e]))           e < d/2
//   out[e + d/2] = fp16(fp16(x[e + d/2] * cos[e + d/2]) + fp16(x[e] * sin[e + d/2]))
// The compiler narrows these fp32 ops to fp16 ones (exact: an fp16 product is exact in fp32, and fp32 has the 2p + 2 bits that make the
// double rounding of a sum innocuous) and would then contract the rounded product into the add (v_pk_fma_f16), which rounds once where
// torch rounds twice: contraction is switched off in qqq_rope_half.  v is copied bit for bit.
#ifndef QQQ_AMD_QQQ_ATTN_HIP_H_
#define QQQ_AMD_QQQ_ATTN_HIP_H_

__device__ __forceinline__ h8 qqq_rope_half(const h8 a, const h8 b, const h8 c, const h8 s, const float sign) {
  // fp16(fp16(a * c) + fp16((sign * b) * s)) per element; sign = -1 for the first half (rotate_half negates x[d/2:]), +1 for the second
#pragma clang fp contract(off)
  h8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const _Float16 p0 = (_Float16)((float)a[e] * (float)c[e]);
    const _Float16 p1 = (_Float16)((sign * (float)b[e]) * (float)s[e]);
    o[e] = (_Float16)((float)p0 + (float)p1);
  }
  return o;
}

template <int NT>
__global__ __launch_bounds__(NT) void qqq_rope_qkv_kernel(const _Float16* __restrict__ q, const int ld_q, const _Float16* __restrict__ k,
                                                          const int ld_k, const _Float16* __restrict__ v, const int ld_v,
                                                          const _Float16* __restrict__ cos_t, const _Float16* __restrict__ sin_t,
                                                          const long long* __restrict__ pos, const long long limit,
                                                          _Float16* __restrict__ q_out, _Float16* __restrict__ k_cache,
                                                          _Float16* __restrict__ v_cache, const int s, const int h, const int kvh,
                                                          const int d, const int cap) {
  const int t = blockIdx.x;  // token bi * s + si
  const long long p = pos[t];
  if (p < 0 || p >= limit) return;  // nothing of this token is written
  const int P = d >> 4;             // items per head
  const int item = blockIdx.y * NT + threadIdx.x;
  if (item >= (h + 2 * kvh) * P) return;
  const int bi = t / s, si = t - bi * s;
  const int hd = d >> 1;
  int head = item / P;
  const int j = (item - head * P) * 8;  // element offset of this lane's vector in the first half-head
  const _Float16* src;
  _Float16* dst;
  if (head < h) {
    src = q + (size_t)t * ld_q + (size_t)head * d;
    dst = q_out + (((size_t)bi * h + head) * s + si) * d;
  } else if (head < h + kvh) {
    head -= h;
    src = k + (size_t)t * ld_k + (size_t)head * d;
    dst = k_cache + (((size_t)bi * kvh + head) * cap + p) * d;
  } else {
    head -= h + kvh;
    const h8* vs = reinterpret_cast<const h8*>(v + (size_t)t * ld_v + (size_t)head * d + j);
    h8* vd = reinterpret_cast<h8*>(v_cache + (((size_t)bi * kvh + head) * cap + p) * d + j);
    const h8 a = vs[0], b = vs[hd >> 3];
    vd[0] = a;
    vd[hd >> 3] = b;
    return;
  }
  const h8 x1 = *reinterpret_cast<const h8*>(src + j), x2 = *reinterpret_cast<const h8*>(src + hd + j);
  const _Float16* cr = cos_t + (size_t)p * d;
  const _Float16* sr = sin_t + (size_t)p * d;
  const h8 c1 = *reinterpret_cast<const h8*>(cr + j), c2 = *reinterpret_cast<const h8*>(cr + hd + j);
  const h8 s1 = *reinterpret_cast<const h8*>(sr + j), s2 = *reinterpret_cast<const h8*>(sr + hd + j);
  *reinterpret_cast<h8*>(dst + j) = qqq_rope_half(x1, x2, c1, s1, -1.0f);
  *reinterpret_cast<h8*>(dst + hd + j) = qqq_rope_half(x2, x1, c2, s2, 1.0f);
}

#endif  // QQQ_AMD_QQQ_ATTN_HIP_H_
