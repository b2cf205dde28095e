// qqq_decode.hip.h -- split-K (flash-decoding) attention of one query token per batch row over the static KV cache, with the output
// produced already int8-quantised for o_proj (include/qqq_amd_decode.h).  Part of the single translation unit qqq_w4a8.hip.
//
// Two launches on the caller's stream:
//   split    grid (splits, kvh, b), 4 waves.  One workgroup takes batch row bi, KV head kh and keys [sp*chunk, (sp+1)*chunk) ∩ [0, pos[bi]],
//            for all G = h / kvh query heads of kh at once, so K and V are read exactly once per KV head.  Wave w walks the 32-key blocks
//            w, w + 4, ... of the chunk with its own online softmax; the four waves merge in LDS and the workgroup writes one fp32 partial
//            (m, l, o[G][d]) per query head to the workspace.  A split that starts beyond pos[bi] exits at once, so the grid is sized by
//            the host's max_len and a captured graph replays at any position below it.
//   combine  grid (b), 512 threads.  Merges the splits covering 0 ... pos[bi] of all h heads (M = max m_i, L = sum l_i 2^(m_i - M),
//            O = sum o_i 2^(m_i - M) / L), rounds O to fp16 once into a row of h*d elements held in registers, optionally stores it, and
//            quantises it with qqq_act_quant_row -- so (xq, s1) is bit for bit dynamic_quant of that fp16 row.
//
// Arithmetic: scores (q.k) * scale with fp16 inputs and fp32 accumulation, kept in the log2 domain (scale * log2 e), fp32 softmax, P
// rounded to fp16 for the PV product (l sums the rounded values), fp32 accumulation.  Both products run on v_mfma_f32_16x16x32_f16 with
// the G query rows padded to 16 (the padding rows hold q = 0 and are never stored):
//   S^T = K Q^T    A = 16 keys x 32 head elements straight from one 16-byte load per lane (lane l: key l&15, elements 32s + 8(l>>4) + j),
//                  B = Q^T (lane l: query row l&15); C leaves query row l&15 on the lane and keys 4(l>>4) + r in its registers, so the
//                  softmax row statistics are lane-local plus a reduction over the lanes l, l^16, l^32, l^48.
//   V^T            the PV product sums over keys, which V's [key][d] layout keeps across lanes; one MFMA against a 0/1 selection matrix
//                  per 16 columns turns a V fragment into C[key 4(l>>4) + r][column l&15] -- exactly (fp16 * 1 + 0s in fp32) -- and that
//                  accumulator is the A operand of the next product with no lane movement and no LDS.
//   O^T += V^T P^T A = the selected V^T, B = P^T (both from registers; the k order is the same permutation of the 32 keys in both), C
//                  keeps query row l&15 on the lane, so the online-softmax rescale is a lane-local multiply.
// K and V go straight from HBM to VGPRs (16-byte loads); LDS holds only the four waves' partials of the final merge.  Four waves per SIMD
// (amdgpu_waves_per_eu): without the bound hipcc keeps every selection MFMA's result live at once, 304 registers and one wave per SIMD.
#ifndef QQQ_AMD_QQQ_DECODE_HIP_H_
#define QQQ_AMD_QQQ_DECODE_HIP_H_

typedef float qqq_f4 __attribute__((ext_vector_type(4)));

static constexpr int DEC_WAVES = 4;                         // waves of a split workgroup
static constexpr int DEC_BLOCK = 32;                        // keys a wave takes per step (the k extent of one PV MFMA)
static constexpr int DEC_ROUND = DEC_WAVES * DEC_BLOCK;     // split chunks are multiples of this
static constexpr int DEC_GMAX = 8;                          // query heads per KV head
static constexpr int DEC_COMBINE_NT = 512;

template <int D>
__global__ __launch_bounds__(DEC_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void qqq_decode_split_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ k_cache, const _Float16* __restrict__ v_cache,
    const long long* __restrict__ pos, const long long limit, const float scale_log2, float* __restrict__ ws_o, float* __restrict__ ws_ml,
    const int h, const int kvh, const int cap, const int chunk, const int splits) {
  constexpr int KS = D / 32;  // k-steps of S^T = K Q^T
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
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, qd = lane >> 4;

  h8 qf[KS];  // B operand of S^T: query row c (zero padding for c >= G), head elements 32s + 8qd + j
  {
    const _Float16* qr = q + ((size_t)bi * h + (size_t)kh * G + (c < G ? c : 0)) * D + 8 * qd;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qf[s] = *reinterpret_cast<const h8*>(qr + 32 * s);
      if (c >= G) qf[s] = h8{};
    }
  }
  h8 sel[2];  // selection matrices: column n of half hh takes k index n + 16 hh (lane l holds k = 8qd + j of column c)
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int j = 0; j < 8; ++j) sel[hh][j] = (8 * qd + j == c + 16 * hh) ? (_Float16)1.0f : (_Float16)0.0f;

  qqq_f4 acc[NT16];  // O^T tile n: lane l, register r = O[query c][16n + 4qd + r]
#pragma unroll
  for (int n = 0; n < NT16; ++n) acc[n] = qqq_f4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;  // running max (log2 domain) and this lane's share of the running sum, for query row c
  const size_t head_row = ((size_t)bi * kvh + kh) * (size_t)cap;

  for (long long kb = k0 + (long long)DEC_BLOCK * w; kb <= last; kb += DEC_ROUND) {
    h8 kf[2][KS], vf[2][KS];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      long long key = kb + 16 * t + c;
      key = key > p ? p : key;  // rows past the last key load a valid row; their scores are masked below
      const size_t off = (head_row + (size_t)key) * D + 8 * qd;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        kf[t][s] = *reinterpret_cast<const h8*>(k_cache + off + 32 * s);
        vf[t][s] = *reinterpret_cast<const h8*>(v_cache + off + 32 * s);
      }
    }
    qqq_f4 st[2];  // S^T: lane l, register r of half t = score of query c against key kb + 16t + 4qd + r
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      st[t] = qqq_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) st[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[t][s], qf[s], st[t], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sv = (kb + 16 * t + 4 * qd + r <= last) ? st[t][r] * scale_log2 : -INFINITY;
        st[t][r] = sv;
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
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        // V^T rows d = 32s + 16hh + c of keys kb + 16t + 4qd + r (t = 0, 1), in the key order of pf
        const qqq_f4 z = qqq_f4{0.f, 0.f, 0.f, 0.f};
        const qqq_f4 t0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[0][s], sel[hh], z, 0, 0, 0);
        const qqq_f4 t1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[1][s], sel[hh], z, 0, 0, 0);
        const h8 va = {(_Float16)t0[0], (_Float16)t0[1], (_Float16)t0[2], (_Float16)t0[3],
                       (_Float16)t1[0], (_Float16)t1[1], (_Float16)t1[2], (_Float16)t1[3]};
        acc[2 * s + hh] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pf, acc[2 * s + hh], 0, 0, 0);
      }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);

  // merge the four waves: every wave rescales to the common max, the workgroup sums and writes one partial per query head
  if (qd == 0 && c < G) {
    lds_m[w][c] = m;
    lds_l[w][c] = l;
  }
  __syncthreads();
  if (c < G) {
    float M = lds_m[0][c];
#pragma unroll
    for (int ww = 1; ww < DEC_WAVES; ++ww) M = fmaxf(M, lds_m[ww][c]);
    const float f = exp2f(m - M);  // M is finite (wave 0 has a block); a wave without one has m = -inf and f = 0
#pragma unroll
    for (int n = 0; n < NT16; ++n) *reinterpret_cast<qqq_f4*>(&lds_o[w][c][16 * n + 4 * qd]) = acc[n] * f;
  }
  __syncthreads();
  const size_t part0 = ((size_t)bi * h + (size_t)kh * G) * splits + sp;  // partial (query 0 of kh, split sp); query g adds g * splits
  for (int i = threadIdx.x; i < G * (D / 4); i += DEC_WAVES * 64) {
    const int g = i / (D / 4), e = (i - g * (D / 4)) * 4;
    qqq_f4 o = *reinterpret_cast<const qqq_f4*>(&lds_o[0][g][e]);
#pragma unroll
    for (int ww = 1; ww < DEC_WAVES; ++ww) o += *reinterpret_cast<const qqq_f4*>(&lds_o[ww][g][e]);
    *reinterpret_cast<qqq_f4*>(ws_o + (part0 + (size_t)g * splits) * D + e) = o;
  }
  if (threadIdx.x < G) {
    const int g = threadIdx.x;
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

// The combine of one row: row bi of the partials, whose query sits at position p (0 <= p < the call's max_len).  The body of
// qqq_decode_combine_kernel, shared with the verify chunk's combine (qqq_verify.hip.h), where a row is a token and p its own position.
template <int VPT, int NT>
__device__ __forceinline__ void qqq_decode_combine_row(const float* __restrict__ ws_o, const float* __restrict__ ws_ml, const int bi,
                                                       const long long p, _Float16* __restrict__ o16, int8_t* __restrict__ xq,
                                                       float* __restrict__ s1, const int h, const int d, const int chunk, const int splits,
                                                       float* red_max) {
  const int nsp = (int)(p / chunk) + 1;  // splits that cover 0 ... p
  const int tid = threadIdx.x;
  const int nvec = (h * d) >> 3;
  h8 v[VPT];
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = tid + i * NT;
    if (idx < nvec) {
      const int head = (idx * 8) / d, e0 = idx * 8 - head * d;
      const size_t part = ((size_t)bi * h + head) * splits;
      const float2* ml = reinterpret_cast<const float2*>(ws_ml) + part;
      float M = -INFINITY;
      for (int s = 0; s < nsp; ++s) M = fmaxf(M, ml[s].x);
      float L = 0.f;
      qqq_f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;
      const float* op = ws_o + part * d + e0;
      for (int s = 0; s < nsp; ++s) {
        const float2 t = ml[s];
        const float f = exp2f(t.x - M);
        L += t.y * f;
        o0 += *reinterpret_cast<const qqq_f4*>(op + (size_t)s * d) * f;
        o1 += *reinterpret_cast<const qqq_f4*>(op + (size_t)s * d + 4) * f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[i][e] = (_Float16)(o0[e] / L);
        v[i][e + 4] = (_Float16)(o1[e] / L);
      }
      if (o16) reinterpret_cast<h8*>(o16 + (size_t)bi * h * d)[idx] = v[i];
    }
  }
  if (xq) qqq_act_quant_row<VPT, NT>(v, nvec, xq + (size_t)bi * h * d, s1 + bi, red_max);
}

// One workgroup per batch row: merge the splits of all h heads, round to fp16 once, optionally store the fp16 row, quantise it.
template <int VPT, int NT>
__global__ __launch_bounds__(NT) void qqq_decode_combine_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                                                const long long* __restrict__ pos, const long long limit,
                                                                _Float16* __restrict__ o16, int8_t* __restrict__ xq, float* __restrict__ s1,
                                                                const int h, const int d, const int chunk, const int splits) {
  __shared__ float red_max[NT / 64];
  const int bi = blockIdx.x;
  const long long p = pos[bi];
  if (p < 0 || p >= limit) return;  // out-of-range row: no fp16 row, no xq, no s1
  qqq_decode_combine_row<VPT, NT>(ws_o, ws_ml, bi, p, o16, xq, s1, h, d, chunk, splits, red_max);
}

#endif  // QQQ_AMD_QQQ_DECODE_HIP_H_
