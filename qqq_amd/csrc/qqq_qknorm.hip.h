// qqq_qknorm.hip.h -- the per-head q / k RMSNorm of a Qwen3 attention block, fused into the rotary embedding and KV-cache write
// (include_ops/qqq_amd_qknorm.h).  Part of the single translation unit qqq_w4a8.hip.
//
// One kernel template serves the four entry points: PAGED picks the block pool (a slot per token, token-major q_out) over the static cache
// (the token's position, q_out in SDPA layout), KV8 the int8 rows with their scales over fp16 rows.  The four kernels without the norm
// (qqq_attn.hip.h, qqq_kv8.hip.h, qqq_paged.hip.h) stay as they are; what is shared with them is the arithmetic behind the norm,
// qqq_rope_half and qqq_kv8_quant_head_row, so with the normed row in place of the projection's row every output is theirs bit for bit.
//
// Decomposition: qqq_rope_qkv_kernel's.  A work item is one 16-byte vector of the first half of a head paired with the matching vector
// of the second half, P = d / 16 neighbouring lanes hold a head (d is 64 or 128, P is 4 or 8), items run over the h q heads, the kvh k
// heads, the kvh v heads; grid x = token, grid y = blocks of NT items, one item per lane, no LDS, no loop.
//
// The norm needs the sum of squares of the whole head row, so a q or k item talks to the other P - 1 lanes of its head: an xor butterfly
// over lanes 1, 2 and (P = 8) 4, on doubles.  Every lane of a P-lane group must reach it, or the whole group must have left: each early
// return and the q / k / v branch decides on (token, head) alone, and P divides both the wave size and the item count, so a group is
// never split.  The butterfly is __shfl_xor on the f64 sum (two 32-bit lane permutes a step, at most three steps): the kernel is one
// short dependent chain per lane, latency- not issue-bound, and sixteen f64 multiply-adds and three adds a lane are far below what the
// loads cost.  f64 makes the order of the sum almost irrelevant to the result and cheap to restate; it is still fixed (see the header).
//
// Arithmetic (include_ops/qqq_amd_qknorm.h): ss in f64 in the stated order; var = float(ss / d); rs = 1 / sqrt(var + eps), both correctly
// rounded in f32; n = fp16(x * rs); y = fp16(w * n).  A square of an fp16 number is exact in f64, so contracting it into the add changes
// nothing; no other rounded product feeds an add here, and contraction is switched off all the same.  The square root is sqrtf, which
// the compiler expands to a correctly rounded sequence (__fsqrt_rn is the bare approximate instruction in this toolchain).
#ifndef QQQ_AMD_QQQ_QKNORM_HIP_H_
#define QQQ_AMD_QQQ_QKNORM_HIP_H_

// Qwen3RMSNorm of one head row spread over P neighbouring lanes, 16 elements a lane (x1 = elements j .. j+7, x2 = d/2 + j .. d/2 + j+7,
// w1 / w2 the weight at the same elements), in place.  Every lane of the P-lane group must be here.
__device__ __forceinline__ void qqq_qknorm_head_row(h8& x1, h8& x2, const h8 w1, const h8 w2, const int P, const float eps) {
#pragma clang fp contract(off)
  double ss = 0.0;
#pragma unroll
  for (int e = 0; e < 8; ++e) ss += (double)x1[e] * (double)x1[e];
#pragma unroll
  for (int e = 0; e < 8; ++e) ss += (double)x2[e] * (double)x2[e];
  ss += __shfl_xor(ss, 1);
  ss += __shfl_xor(ss, 2);
  if (P == 8) ss += __shfl_xor(ss, 4);                           // P is uniform over the launch
  const float var = (float)(ss * (P == 8 ? 1.0 / 128 : 1.0 / 64));  // ss / d, exactly: d = 16 P is a power of two
  const float rs = __frcp_rn(sqrtf(var + eps));
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const _Float16 n1 = (_Float16)((float)x1[e] * rs), n2 = (_Float16)((float)x2[e] * rs);
    x1[e] = (_Float16)((float)w1[e] * (float)n1);
    x2[e] = (_Float16)((float)w2[e] * (float)n2);
  }
}

// where: the static cache's row length `cap` (PAGED = false), or log2 of the pool's block size (PAGED = true); slots / nslots and
// k_scale / v_scale are read only where PAGED / KV8 says so.  k_dst / v_dst are fp16 or int8 rows of d elements.
template <int NT, bool PAGED, bool KV8>
__global__ __launch_bounds__(NT) void qqq_rope_qkv_norm_kernel(
    const _Float16* __restrict__ q, const int ld_q, const _Float16* __restrict__ k, const int ld_k, const _Float16* __restrict__ v,
    const int ld_v, const _Float16* __restrict__ q_weight, const _Float16* __restrict__ k_weight, const float eps,
    const _Float16* __restrict__ cos_t, const _Float16* __restrict__ sin_t, const long long* __restrict__ pos, const long long limit,
    const long long* __restrict__ slots, const long long nslots, _Float16* __restrict__ q_out, void* __restrict__ k_dst,
    void* __restrict__ v_dst, float* __restrict__ k_scale, float* __restrict__ v_scale, const int s, const int h, const int kvh, const int d,
    const int where) {
  const int t = blockIdx.x;  // token (bi * s + si in the static cache)
  const long long p = pos[t];
  if (p < 0 || p >= limit) return;  // nothing of this token is written (the whole workgroup leaves)
  const int P = d >> 4;             // items per head: 4 or 8, so a head's lanes are neighbours in one wave
  const int item = blockIdx.y * NT + threadIdx.x;
  if (item >= (h + 2 * kvh) * P) return;  // whole heads: (h + 2 kvh) P is a multiple of P
  const int hd = d >> 1;
  const int head = item / P;
  const int j = (item - head * P) * 8;  // element offset of this lane's vector in the first half-head
  long long slot = p;
  if (PAGED) {
    slot = slots[t];
    if (head >= h && (slot < 0 || slot >= nslots)) return;  // a padding slot: the token's q_out row only (whole heads leave together)
  }
  const bool is_q = head < h, is_v = head >= h + kvh;
  h8 lo, hi;
  if (is_v) {  // plain
    const h8* vs = reinterpret_cast<const h8*>(v + (size_t)t * ld_v + (size_t)(head - h - kvh) * d + j);
    lo = vs[0];
    hi = vs[hd >> 3];
  } else {  // q or k: normed, then rotated (whole heads are here: the butterfly's partners are too)
    const _Float16* src = is_q ? q + (size_t)t * ld_q + (size_t)head * d : k + (size_t)t * ld_k + (size_t)(head - h) * d;
    const _Float16* wr = is_q ? q_weight : k_weight;
    h8 x1 = *reinterpret_cast<const h8*>(src + j), x2 = *reinterpret_cast<const h8*>(src + hd + j);
    const h8 w1 = *reinterpret_cast<const h8*>(wr + j), w2 = *reinterpret_cast<const h8*>(wr + hd + j);
    const _Float16* cr = cos_t + (size_t)p * d;
    const _Float16* sr = sin_t + (size_t)p * d;
    const h8 c1 = *reinterpret_cast<const h8*>(cr + j), c2 = *reinterpret_cast<const h8*>(cr + hd + j);
    const h8 s1 = *reinterpret_cast<const h8*>(sr + j), s2 = *reinterpret_cast<const h8*>(sr + hd + j);
    qqq_qknorm_head_row(x1, x2, w1, w2, P, eps);
    lo = qqq_rope_half(x1, x2, c1, s1, -1.0f);
    hi = qqq_rope_half(x2, x1, c2, s2, 1.0f);
  }
  if (is_q) {
    size_t row;
    if (PAGED) {
      row = (size_t)t * h + head;
    } else {
      const int bi = t / s, si = t - bi * s;
      row = ((size_t)bi * h + head) * s + si;
    }
    *reinterpret_cast<h8*>(q_out + row * d + j) = lo;
    *reinterpret_cast<h8*>(q_out + row * d + hd + j) = hi;
    return;
  }
  const int hk = head - (is_v ? h + kvh : h);
  size_t row;
  if (PAGED)
    row = (((size_t)(slot >> where) * kvh + hk) << where) + (size_t)(slot & ((1 << where) - 1));
  else
    row = ((size_t)(t / s) * kvh + hk) * where + (size_t)p;
  if (KV8) {
    qqq_kv8_quant_head_row(lo, hi, P, j, hd, static_cast<int8_t*>(is_v ? v_dst : k_dst) + row * d, (is_v ? v_scale : k_scale) + row);
  } else {
    _Float16* dst = static_cast<_Float16*>(is_v ? v_dst : k_dst) + row * d;
    *reinterpret_cast<h8*>(dst + j) = lo;
    *reinterpret_cast<h8*>(dst + hd + j) = hi;
  }
}

#endif  // QQQ_AMD_QQQ_QKNORM_HIP_H_
