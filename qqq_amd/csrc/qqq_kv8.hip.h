// qqq_kv8.hip.h -- the int8 KV cache (include/qqq_amd_kv8.h): the RoPE / cache-write kernel that quantises each head row as it stores it,
// and the split kernel of the decode attention that reads those rows.  Part of the single translation unit qqq_w4a8.hip.
//
// A cached head row (one token, one KV head, d elements) is dynamic_quant of the fp16 row the fp16 cache would hold: d int8 codes in
// k_cache / v_cache [b, kvh, cap, d] and one fp32 scale in k_scale / v_scale [b, kvh, cap]; d + 4 bytes against 2 d.
//
//   qqq_kv8_rope_qkv_kernel      qqq_rope_qkv_kernel's item layout (one lane = a 16-byte vector of the first half of a head and the matching
//                                vector of the second half; P = d / 16 neighbouring lanes hold a head).  q items are written as there.  A k
//                                or v item keeps its 16 fp16 elements in registers, the row's amax is a reduction over the P lanes (xor
//                                shuffles, no LDS), and the quantisation step is qqq_act_quant_row's, element for element.
//   qqq_kv8_decode_split_kernel  qqq_decode_split_kernel with int8 K and V: same grid, chunking, online softmax, LDS merge and workspace
//                                layout, so qqq_decode_combine_kernel finishes the call unchanged.  One 16-byte load per lane now holds 16
//                                elements of a key (lane l: key l&15, elements 64 g + 16 (l>>4) + j of the 64-element segment g).
//     S^T = K Q^T   the codes become fp16 exactly (bias trick: 0x6400 | (code ^ 0x80) is 1024 + code + 128) and feed the same
//                   v_mfma_f32_16x16x32_f16 as the fp16 kernel, bytes 0..7 of the load in one k-step and 8..15 in the next; Q^T is read in
//                   that element order from LDS, where the workgroup puts it once (in registers it would take D / 8 of the 128 a wave has
//                   at four waves per SIMD).  The fp32 score is then multiplied by k_scale[key] * scale * log2 e.
//     V^T           v_mfma_i32_16x16x64_i8 of the raw load against a 0/1 byte selection matrix gives C[key 4(l>>4) + r][column l&15] as
//                   exact int32; it is multiplied by v_scale[key] in fp32 and rounded to fp16 once -- the probabilities never carry a
//                   value scale, so small scales cannot underflow in them.
//     O^T += V^T P^T  as in the fp16 kernel.
//   K / V loads are non-temporal (each byte is read once per call); the per-key scales are read as 16-byte vectors when cap and the scale
//   pointers allow it, as four dwords otherwise.  Keys past the row's last one load the last key's codes, score -inf and a value scale of 0.
//   A block's first key is wave-uniform, so its addresses are a scalar base plus 32-bit lane offsets.
#ifndef QQQ_AMD_QQQ_KV8_HIP_H_
#define QQQ_AMD_QQQ_KV8_HIP_H_

// dynamic_quant of one head row spread over P neighbouring lanes, 16 elements a lane (lo = elements j .. j+7, hi = d/2 + j .. d/2 + j+7);
// the arithmetic of qqq_act_quant_row.  Every lane of the P-lane group must be here.
__device__ __forceinline__ void qqq_kv8_quant_head_row(const h8 lo, const h8 hi, const int P, const int j, const int hd,
                                                       int8_t* __restrict__ codes, float* __restrict__ scale_slot) {
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fmaxf(fabsf((float)lo[e]), fabsf((float)hi[e])));
  amax = fmaxf(amax, __shfl_xor(amax, 1));
  amax = fmaxf(amax, __shfl_xor(amax, 2));
  if (P == 8) amax = fmaxf(amax, __shfl_xor(amax, 4));  // P is uniform over the launch
  const float scale = (float)(_Float16)__fmul_rn(amax, 1.0f / 127.0f);
  if (j == 0) *scale_slot = scale;
  const float rinv = (scale > 0.f) ? __frcp_rn(scale) : 0.f;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const h8 x = half ? hi : lo;
    unsigned w[2] = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xe = (float)x[e];
      const float p = xe * rinv;
      float qv = rintf(p);
      const bool near_tie = fabsf(p - qv) > 0.4995f;
      if (__builtin_amdgcn_ballot_w64(near_tie) != 0) {
        const float qd = (scale > 0.f) ? rintf(__fdiv_rn(xe, scale)) : 0.f;
        qv = near_tie ? qd : qv;
      }
      w[e >> 2] |= ((unsigned)((int)fminf(fmaxf(qv, -128.f), 127.f)) & 0xFFu) << (8 * (e & 3));
    }
    *reinterpret_cast<int2*>(codes + (half ? hd : 0) + j) = make_int2((int)w[0], (int)w[1]);
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void qqq_kv8_rope_qkv_kernel(const _Float16* __restrict__ q, const int ld_q, const _Float16* __restrict__ k,
                                                              const int ld_k, const _Float16* __restrict__ v, const int ld_v,
                                                              const _Float16* __restrict__ cos_t, const _Float16* __restrict__ sin_t,
                                                              const long long* __restrict__ pos, const long long limit,
                                                              _Float16* __restrict__ q_out, int8_t* __restrict__ k_cache,
                                                              int8_t* __restrict__ v_cache, float* __restrict__ k_scale,
                                                              float* __restrict__ v_scale, const int s, const int h, const int kvh,
                                                              const int d, const int cap) {
  const int t = blockIdx.x;  // token bi * s + si
  const long long p = pos[t];
  if (p < 0 || p >= limit) return;  // nothing of this token is written
  const int P = d >> 4;             // items per head: 4 or 8, so a head's lanes are neighbours in one wave
  const int item = blockIdx.y * NT + threadIdx.x;
  if (item >= (h + 2 * kvh) * P) return;  // whole heads: (h + 2 kvh) P is a multiple of P
  const int bi = t / s, si = t - bi * s;
  const int hd = d >> 1;
  int head = item / P;
  const int j = (item - head * P) * 8;  // element offset of this lane's vector in the first half-head
  h8 lo, hi;
  if (head >= h + kvh) {  // v: plain
    const h8* vs = reinterpret_cast<const h8*>(v + (size_t)t * ld_v + (size_t)(head - h - kvh) * d + j);
    lo = vs[0];
    hi = vs[hd >> 3];
  } else {  // q or k: rotated
    const _Float16* src = head < h ? q + (size_t)t * ld_q + (size_t)head * d : k + (size_t)t * ld_k + (size_t)(head - h) * d;
    const h8 x1 = *reinterpret_cast<const h8*>(src + j), x2 = *reinterpret_cast<const h8*>(src + hd + j);
    const _Float16* cr = cos_t + (size_t)p * d;
    const _Float16* sr = sin_t + (size_t)p * d;
    const h8 c1 = *reinterpret_cast<const h8*>(cr + j), c2 = *reinterpret_cast<const h8*>(cr + hd + j);
    const h8 s1 = *reinterpret_cast<const h8*>(sr + j), s2 = *reinterpret_cast<const h8*>(sr + hd + j);
    lo = qqq_rope_half(x1, x2, c1, s1, -1.0f);
    hi = qqq_rope_half(x2, x1, c2, s2, 1.0f);
  }
  if (head < h) {
    _Float16* dst = q_out + (((size_t)bi * h + head) * s + si) * d;
    *reinterpret_cast<h8*>(dst + j) = lo;
    *reinterpret_cast<h8*>(dst + hd + j) = hi;
    return;
  }
  const bool is_v = head >= h + kvh;
  head -= is_v ? h + kvh : h;
  const size_t row = ((size_t)bi * kvh + head) * cap + (size_t)p;
  qqq_kv8_quant_head_row(lo, hi, P, j, hd, (is_v ? v_cache : k_cache) + row * d, (is_v ? v_scale : k_scale) + row);
}

// 8 int8 codes (two dwords) -> 8 fp16, exactly: byte b ^ 0x80 under the exponent byte 0x64 is the fp16 number 1024 + code + 128
__device__ __forceinline__ h8 qqq_kv8_codes_to_h8(const int w0, const int w1) {
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  const unsigned a = (unsigned)w0 ^ 0x80808080u, b = (unsigned)w1 ^ 0x80808080u;
  const u4v bits = {__builtin_amdgcn_perm(0x64646464u, a, 0x04010400u), __builtin_amdgcn_perm(0x64646464u, a, 0x04030402u),
                    __builtin_amdgcn_perm(0x64646464u, b, 0x04010400u), __builtin_amdgcn_perm(0x64646464u, b, 0x04030402u)};
  h8 x = __builtin_bit_cast(h8, bits);
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] -= (_Float16)1152.0f;
  return x;
}

template <int D>
__global__ __launch_bounds__(DEC_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void qqq_kv8_decode_split_kernel(
    const _Float16* __restrict__ q, const int8_t* __restrict__ k_cache, const int8_t* __restrict__ v_cache,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale, const long long* __restrict__ pos, const long long limit,
    const float scale_log2, float* __restrict__ ws_o, float* __restrict__ ws_ml, const int h, const int kvh, const int cap, const int chunk,
    const int splits) {
  constexpr int SG = D / 64;    // 64-element segments of a head row: one 16-byte load per lane each
  constexpr int NT16 = D / 16;  // 16-column tiles of O^T
  __shared__ float lds_o[DEC_WAVES][DEC_GMAX][D];
  __shared__ float lds_m[DEC_WAVES][DEC_GMAX], lds_l[DEC_WAVES][DEC_GMAX];
  const int sp = blockIdx.x, kh = blockIdx.y, bi = blockIdx.z;
  const long long p = pos[bi];
  if (p < 0 || p >= limit) return;  // out-of-range row: nothing is written
  const long long k0 = (long long)sp * chunk;
  if (k0 > p) return;  // the split lies wholly beyond this row's last key
  const long long last = (k0 + chunk - 1 < p) ? k0 + chunk - 1 : p;
  const int G = h / kvh;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform and known to be: a block's addresses stay in SGPRs
  const int c = lane & 15, qd = lane >> 4;

  // Q^T, the B operand of S^T, waits in LDS (in the space of lds_o, which is not written before the loop is over): query row c of 16
  // (zeros for c >= G), rows padded by 8 elements against bank conflicts.  In registers it would cost D / 8 of the 128 a wave has.
  constexpr int QLD = D + 8;
  _Float16* lds_q = reinterpret_cast<_Float16*>(&lds_o[0][0][0]);
  static_assert(16 * (D / 8) <= DEC_WAVES * 64, "one 16-byte vector of Q^T per thread");
  if (threadIdx.x < 16 * (D / 8)) {
    const int row = threadIdx.x / (D / 8), e = (threadIdx.x - row * (D / 8)) * 8;
    h8 x = h8{};
    if (row < G) x = *reinterpret_cast<const h8*>(q + ((size_t)bi * h + (size_t)kh * G + row) * D + e);
    *reinterpret_cast<h8*>(lds_q + row * QLD + e) = x;
  }
  __syncthreads();
  const _Float16* qrow = lds_q + c * QLD + 16 * qd;  // elements 64g + 16qd + 8u + j: the order of a K load's bytes
  v4i onehot;  // byte c of the lane's 16
#pragma unroll
  for (int i = 0; i < 4; ++i) onehot[i] = ((c >> 2) == i) ? (1 << (8 * (c & 3))) : 0;

  qqq_f4 acc[NT16];  // O^T tile n: lane l, register r = O[query c][16n + 4qd + r]
#pragma unroll
  for (int n = 0; n < NT16; ++n) acc[n] = qqq_f4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;  // running max (log2 domain) and this lane's share of the running sum, for query row c
  const size_t head_row = ((size_t)bi * kvh + kh) * (size_t)cap;
  // 16-byte scale loads need every head row of scales 16-byte aligned and a multiple of four keys long
  const bool vec_scales = (cap & 3) == 0 && (((uintptr_t)k_scale | (uintptr_t)v_scale) & 15) == 0;

  for (long long kb = k0 + (long long)DEC_BLOCK * w; kb <= last; kb += DEC_ROUND) {
    // the block's first key is wave-uniform; a lane adds 32-bit offsets inside the block
    const int8_t* kblk = k_cache + (head_row + (size_t)kb) * D;
    const int8_t* vblk = v_cache + (head_row + (size_t)kb) * D;
    const float* ksb = k_scale + head_row + (size_t)kb;
    const float* vsb = v_scale + head_row + (size_t)kb;
    const int rem = (int)(last - kb < DEC_BLOCK - 1 ? last - kb : DEC_BLOCK - 1);  // the block's last key to attend
    const int pin = (int)(p - kb < DEC_BLOCK - 1 ? p - kb : DEC_BLOCK - 1);        // the row's last key, if it lies in the block
    v4i kr[2][SG], vr[2][SG];
    qqq_f4 ksc[2], vsc[2];  // scales of keys kb + 16t + 4qd + r
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = 16 * t + c < pin ? 16 * t + c : pin;  // rows past the row's last key load that key; their scores are masked below
      const int off = key * D + 16 * qd;
#pragma unroll
      for (int g = 0; g < SG; ++g) {
        kr[t][g] = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(kblk + off + 64 * g));
        vr[t][g] = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(vblk + off + 64 * g));
      }
      const int g0 = 16 * t + 4 * qd;
      if (vec_scales) {
        const int gg = g0 < (pin & ~3) ? g0 : (pin & ~3);  // a clamped group holds masked keys only
        ksc[t] = *reinterpret_cast<const qqq_f4*>(ksb + gg);
        vsc[t] = *reinterpret_cast<const qqq_f4*>(vsb + gg);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kk = g0 + r < pin ? g0 + r : pin;
          ksc[t][r] = ksb[kk];
          vsc[t][r] = vsb[kk];
        }
      }
    }
    qqq_f4 st[2];  // S^T: lane l, register r of half t = score of query c against key kb + 16t + 4qd + r
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      st[t] = qqq_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int g = 0; g < SG; ++g) {
        const h8 q0 = *reinterpret_cast<const h8*>(qrow + 64 * g), q1 = *reinterpret_cast<const h8*>(qrow + 64 * g + 8);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qqq_kv8_codes_to_h8(kr[t][g][0], kr[t][g][1]), q0, st[t], 0, 0, 0);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qqq_kv8_codes_to_h8(kr[t][g][2], kr[t][g][3]), q1, st[t], 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool valid = 4 * qd <= rem - (16 * t + r);  // one lane value against eight wave-uniform ones
        const float sv = valid ? st[t][r] * (ksc[t][r] * scale_log2) : -INFINITY;
        st[t][r] = sv;
        vsc[t][r] = valid ? vsc[t][r] : 0.f;  // whatever an unwritten slot holds stays out of the product with P = 0
        mx = fmaxf(mx, sv);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);  // finite: key kb <= last is in every block
    const float alpha = exp2f(m - mn);
    m = mn;
    h8 pf;  // B operand of O^T: P[query c][key kb + 16 (j >> 2) + 4qd + (j & 3)] in fp16
    float ps = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const _Float16 ph = (_Float16)exp2f(st[t][r] - mn);
        pf[4 * t + r] = ph;
        ps += (float)ph;
      }
    l = l * alpha + ps;
#pragma unroll
    for (int n = 0; n < NT16; ++n) acc[n] *= alpha;
    int qdv = qd;
    asm volatile("" : "+v"(qdv));  // see sel below
#pragma unroll
    for (int g = 0; g < SG; ++g)
#pragma unroll
      for (int tl = 0; tl < 4; ++tl) {
        // byte selection matrix: column n of tile tl takes the k slot (lane group tl, byte n), i.e. element 16 tl + n of the segment.  Made
        // here from a lane-group index the compiler cannot see through: hoisted out of the loop the four would hold 16 registers across
        // the loads.
        const v4i sel = (qdv == tl) ? onehot : v4i{0, 0, 0, 0};
        // V^T rows d = 64g + 16tl + c of keys kb + 16t + 4qd + r (t = 0, 1), in the key order of pf: exact int32 codes, times the key's scale
        const v4i z = v4i{0, 0, 0, 0};
        const v4i t0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(vr[0][g], sel, z, 0, 0, 0);
        const v4i t1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(vr[1][g], sel, z, 0, 0, 0);
        const h8 va = {(_Float16)((float)t0[0] * vsc[0][0]), (_Float16)((float)t0[1] * vsc[0][1]), (_Float16)((float)t0[2] * vsc[0][2]),
                       (_Float16)((float)t0[3] * vsc[0][3]), (_Float16)((float)t1[0] * vsc[1][0]), (_Float16)((float)t1[1] * vsc[1][1]),
                       (_Float16)((float)t1[2] * vsc[1][2]), (_Float16)((float)t1[3] * vsc[1][3])};
        acc[4 * g + tl] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pf, acc[4 * g + tl], 0, 0, 0);
        if (tl & 1) __builtin_amdgcn_sched_barrier(0);  // two tiles in flight: all sixteen selection results at once do not fit 128 registers
      }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);

  // merge the four waves and write one partial per query head: the layout qqq_decode_split_kernel leaves for qqq_decode_combine_kernel.
  // The lane indices are taken afresh, so that the addresses below are worked out here and not carried through the loop in registers.
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int ce = tid & 15, qe = (tid >> 4) & 3;
  if (qe == 0 && ce < G) {
    lds_m[w][ce] = m;
    lds_l[w][ce] = l;
  }
  __syncthreads();
  if (ce < G) {
    float M = lds_m[0][ce];
#pragma unroll
    for (int ww = 1; ww < DEC_WAVES; ++ww) M = fmaxf(M, lds_m[ww][ce]);
    const float f = exp2f(m - M);  // M is finite (wave 0 has a block); a wave without one has m = -inf and f = 0
#pragma unroll
    for (int n = 0; n < NT16; ++n) *reinterpret_cast<qqq_f4*>(&lds_o[w][ce][16 * n + 4 * qe]) = acc[n] * f;
  }
  __syncthreads();
  const size_t part0 = ((size_t)bi * h + (size_t)kh * G) * splits + sp;  // partial (query 0 of kh, split sp); query g adds g * splits
  for (int i = tid; i < G * (D / 4); i += DEC_WAVES * 64) {
    const int g = i / (D / 4), e = (i - g * (D / 4)) * 4;
    qqq_f4 o = *reinterpret_cast<const qqq_f4*>(&lds_o[0][g][e]);
#pragma unroll
    for (int ww = 1; ww < DEC_WAVES; ++ww) o += *reinterpret_cast<const qqq_f4*>(&lds_o[ww][g][e]);
    *reinterpret_cast<qqq_f4*>(ws_o + (part0 + (size_t)g * splits) * D + e) = o;
  }
  if (tid < G) {
    const int g = tid;
    float M = lds_m[0][g];
#pragma unroll
    for (int ww = 1; ww < DEC_WAVES; ++ww) M = fmaxf(M, lds_m[ww][g]);
    float L = 0.f;
#pragma unroll
    for (int ww = 0; ww < DEC_WAVES; ++ww) L += lds_l[ww][g] * exp2f(lds_m[ww][g] - M);
    float2* ml = reinterpret_cast<float2*>(ws_ml) + part0 + (size_t)g * splits;
    *ml = make_float2(M, L);
  }
}

#endif  // QQQ_AMD_QQQ_KV8_HIP_H_
