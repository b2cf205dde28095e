// qqq_window.hip.h -- sliding-window attention over the block pools (include/qqq_amd_window.h): a query at position i attends the W keys
// lo(i) = max(0, i - W + 1) ... i.  The windowed twins of the paged split-K decode kernels (qqq_paged.hip.h) and of the paged prefill
// kernel (qqq_prefill.hip.h): their arithmetic, operand layouts and order of sums, another split of the work.  Part of the single
// translation unit qqq_w4a8.hip.
//
//   qqq_window_decode_split_kernel       grid (splits, kvh, b), 4 waves, the plan made over span = min(max_len, round_up(W + DEC_ROUND - 1))
//   qqq_window_kv8_decode_split_kernel   keys, not over max_len: a step costs O(W).  Every row places its splits itself: base = lo(pos)
//                                        rounded down to DEC_ROUND, split sp owns [base + sp * chunk, base + (sp + 1) * chunk) ∩ [lo, pos].
//                                        lo lies in split 0 (base <= lo < base + DEC_ROUND <= base + chunk), so the splits that write are
//                                        0 ... (pos - base) / chunk, and pos - base < span keeps that below `splits`.  A wave's 32-key
//                                        steps stay aligned to the absolute key index; a step wholly below lo is skipped (only the first
//                                        round of split 0 can hold one).  A key of a step outside [lo, pos] is clamped into it before the
//                                        load and its score is masked, on both sides the same way; the block id of a 16-key half is
//                                        that of its first key clamped into [lo, pos], which is the block of every key the half loads.
//                                        With lo = 0: base 0, the plain kernels' chunks, steps and sums -- their partials bit for bit.
//   qqq_window_decode_combine_kernel     qqq_decode_combine_row over the splits 0 ... (pos - base) / chunk of a row.
//   qqq_window_prefill_attn_kernel       qqq_prefill_attn_kernel's query tiles, staging and MFMA loop; the 64-key tiles are walked from the
//                                        one that holds lo(first token of the tile), nothing before it is loaded and its table entries
//                                        are not read.  A row's band lo(pos) ... pos is a mask on both sides; a wave skips the steps
//                                        wholly below the band of its first row or above its last row's position.
//     masked step   later rows of a tile have a higher lo than its first row, so a row can meet steps in which it attends nothing while
//                   its running max is still -inf.  Such a step is an exact no-op: the max the exponents are taken against is 0 where
//                   the new running max is -inf (alpha = 2^-inf = 0 on a zero state, P = 2^(-inf - 0) = 0), and the new max itself
//                   where it is finite -- the plain kernel's arithmetic, bit for bit.
#ifndef QQQ_AMD_QQQ_WINDOW_HIP_H_
#define QQQ_AMD_QQQ_WINDOW_HIP_H_

// the first key a query at position p attends
__device__ __forceinline__ long long qqq_window_lo(const long long p, const int window) {
  const long long lo = p - window + 1;
  return lo > 0 ? lo : 0;
}

// the block row of the 16-key half that starts at `key`, for a row attending [lo, p]: every key the half loads is clamped into [lo, p],
// and so is the key whose table entry is read -- entries below lo / block_size and above p / block_size never are
__device__ __forceinline__ size_t qqq_window_block_row(const int* __restrict__ table, long long key, const long long lo, const long long p,
                                                       const int lbs, const int num_blocks, const int kvh, const int kh) {
  key = key < lo ? lo : (key > p ? p : key);
  return qqq_paged_block_row(table, key, lbs, num_blocks, kvh, kh);
}

// The end of a split workgroup: merge the four waves' (m, l, acc) in LDS and write one fp32 partial per query head, in the layout and
// with the order of sums of qqq_paged_decode_split_kernel.  `l` is already summed over the wave.  The lane indices are taken afresh, so
// that the addresses are worked out here and not carried through the key loop in registers.
template <int D>
__device__ __forceinline__ void qqq_window_write_partial(float (&lds_o)[DEC_WAVES][DEC_GMAX][D], float (&lds_m)[DEC_WAVES][DEC_GMAX],
                                                         float (&lds_l)[DEC_WAVES][DEC_GMAX], const qqq_f4 (&acc)[D / 16], const float m,
                                                         const float l, const int w, const int G, const size_t part0, const int splits,
                                                         float* __restrict__ ws_o, float* __restrict__ ws_ml) {
  constexpr int NT16 = D / 16;
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
    const float f = exp2f(m - M);  // M is finite (some wave has a step with a key of [lo, pos]); a wave without one has m = -inf and f = 0
#pragma unroll
    for (int n = 0; n < NT16; ++n) *reinterpret_cast<qqq_f4*>(&lds_o[w][ce][16 * n + 4 * qe]) = acc[n] * f;
  }
  __syncthreads();
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

template <int D>
__global__ __launch_bounds__(DEC_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void qqq_window_decode_split_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ k_pool, const _Float16* __restrict__ v_pool,
    const int* __restrict__ block_table, const int table_stride, const long long* __restrict__ pos, const long long limit, const int window,
    const float scale_log2, float* __restrict__ ws_o, float* __restrict__ ws_ml, const int h, const int kvh, const int num_blocks,
    const int lbs, const int chunk, const int splits) {
  constexpr int KS = D / 32;    // k-steps of S^T = K Q^T
  constexpr int NT16 = D / 16;  // 16-column tiles of O^T
  __shared__ float lds_o[DEC_WAVES][DEC_GMAX][D];
  __shared__ float lds_m[DEC_WAVES][DEC_GMAX], lds_l[DEC_WAVES][DEC_GMAX];
  const int sp = blockIdx.x, kh = blockIdx.y, bi = blockIdx.z;
  const long long p = pos[bi];
  if (p < 0 || p >= limit) return;  // out-of-range row: nothing is written
  const long long lo = qqq_window_lo(p, window);
  const long long k0 = (lo & ~(long long)(DEC_ROUND - 1)) + (long long)sp * chunk;  // the row's own placement: split 0 starts at lo's round
  if (k0 > p) return;  // the split lies wholly beyond this row's last key (none lies wholly below lo: lo is in split 0)
  const long long first = k0 > lo ? k0 : lo;
  const long long last = (k0 + chunk - 1 < p) ? k0 + chunk - 1 : p;
  const int G = h / kvh;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform and known to be: the table loads are scalar
  const int c = lane & 15, qd = lane >> 4;
  const int* table = block_table + (size_t)bi * table_stride;
  const int bmask = (1 << lbs) - 1;

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

  long long kb = k0 + (long long)DEC_BLOCK * w;
  if (kb + DEC_BLOCK - 1 < first) kb += DEC_ROUND;  // the wave's step of the first round lies wholly below lo: every later one holds a key
  size_t nrow[2] = {0, 0};  // block rows of the two 16-key halves of a step, fetched one step ahead
  if (kb <= last) {
    nrow[0] = qqq_window_block_row(table, kb, lo, p, lbs, num_blocks, kvh, kh);
    nrow[1] = lbs >= 5 ? nrow[0] : qqq_window_block_row(table, kb + 16, lo, p, lbs, num_blocks, kvh, kh);
  }
  for (; kb <= last; kb += DEC_ROUND) {
    const size_t brow[2] = {nrow[0], nrow[1]};
    const long long nk = kb + DEC_ROUND;
    if (nk <= last) {
      nrow[0] = qqq_window_block_row(table, nk, lo, p, lbs, num_blocks, kvh, kh);
      nrow[1] = lbs >= 5 ? nrow[0] : qqq_window_block_row(table, nk + 16, lo, p, lbs, num_blocks, kvh, kh);
    }
    h8 kf[2][KS], vf[2][KS];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      long long key = kb + 16 * t + c;
      key = key > p ? p : key;    // rows outside [lo, p] load a valid row of the window; their scores are masked below
      key = key < lo ? lo : key;
      const int off = ((int)key & bmask) * D + 8 * qd;
      const _Float16* kblk = k_pool + brow[t] * D;
      const _Float16* vblk = v_pool + brow[t] * D;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        kf[t][s] = *reinterpret_cast<const h8*>(kblk + off + 32 * s);
        vf[t][s] = *reinterpret_cast<const h8*>(vblk + off + 32 * s);
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
        const long long kk = kb + 16 * t + 4 * qd + r;
        const float sv = (kk <= last && kk >= first) ? st[t][r] * scale_log2 : -INFINITY;
        st[t][r] = sv;
        mx = fmaxf(mx, sv);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);  // finite: every step that is walked holds a key of [first, last]
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
  const size_t part0 = ((size_t)bi * h + (size_t)kh * G) * splits + sp;  // partial (query 0 of kh, split sp); query g adds g * splits
  qqq_window_write_partial<D>(lds_o, lds_m, lds_l, acc, m, l, w, G, part0, splits, ws_o, ws_ml);
}

template <int D>
__global__ __launch_bounds__(DEC_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void qqq_window_kv8_decode_split_kernel(
    const _Float16* __restrict__ q, const int8_t* __restrict__ k_pool, const int8_t* __restrict__ v_pool, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, const int* __restrict__ block_table, const int table_stride, const long long* __restrict__ pos,
    const long long limit, const int window, const float scale_log2, float* __restrict__ ws_o, float* __restrict__ ws_ml, const int h,
    const int kvh, const int num_blocks, const int lbs, const int chunk, const int splits) {
  constexpr int SG = D / 64;    // 64-element segments of a head row: one 16-byte load per lane each
  constexpr int NT16 = D / 16;  // 16-column tiles of O^T
  __shared__ float lds_o[DEC_WAVES][DEC_GMAX][D];
  __shared__ float lds_m[DEC_WAVES][DEC_GMAX], lds_l[DEC_WAVES][DEC_GMAX];
  const int sp = blockIdx.x, kh = blockIdx.y, bi = blockIdx.z;
  const long long p = pos[bi];
  if (p < 0 || p >= limit) return;  // out-of-range row: nothing is written
  const long long lo = qqq_window_lo(p, window);
  const long long k0 = (lo & ~(long long)(DEC_ROUND - 1)) + (long long)sp * chunk;  // the row's own placement: split 0 starts at lo's round
  if (k0 > p) return;  // the split lies wholly beyond this row's last key (none lies wholly below lo: lo is in split 0)
  const long long first = k0 > lo ? k0 : lo;
  const long long last = (k0 + chunk - 1 < p) ? k0 + chunk - 1 : p;
  const int G = h / kvh;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform and known to be: a block's addresses stay in SGPRs
  const int c = lane & 15, qd = lane >> 4;
  const int* table = block_table + (size_t)bi * table_stride;
  const int bmask = (1 << lbs) - 1;

  // Q^T, the B operand of S^T, waits in LDS (in the space of lds_o, which is not written before the loop is over), as in
  // qqq_paged_kv8_decode_split_kernel: query row c of 16 (zeros for c >= G), rows padded by 8 elements against bank conflicts.
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
  // 16-byte scale loads need the scale pools 16-byte aligned: a (block, head) row of scales is block_size >= 16 floats long
  const bool vec_scales = (((uintptr_t)k_scale | (uintptr_t)v_scale) & 15) == 0;

  long long kb = k0 + (long long)DEC_BLOCK * w;
  if (kb + DEC_BLOCK - 1 < first) kb += DEC_ROUND;  // the wave's step of the first round lies wholly below lo: every later one holds a key
  size_t nrow[2] = {0, 0};  // block rows of the two 16-key halves of a step, fetched one step ahead
  if (kb <= last) {
    nrow[0] = qqq_window_block_row(table, kb, lo, p, lbs, num_blocks, kvh, kh);
    nrow[1] = lbs >= 5 ? nrow[0] : qqq_window_block_row(table, kb + 16, lo, p, lbs, num_blocks, kvh, kh);
  }
  for (; kb <= last; kb += DEC_ROUND) {
    const size_t brow[2] = {nrow[0], nrow[1]};
    const long long nk = kb + DEC_ROUND;
    if (nk <= last) {
      nrow[0] = qqq_window_block_row(table, nk, lo, p, lbs, num_blocks, kvh, kh);
      nrow[1] = lbs >= 5 ? nrow[0] : qqq_window_block_row(table, nk + 16, lo, p, lbs, num_blocks, kvh, kh);
    }
    const int kin = (int)kb & bmask;  // the step's first key inside its block (0 where block_size is 16 or 32)
    const int rem = (int)(last - kb < DEC_BLOCK - 1 ? last - kb : DEC_BLOCK - 1);  // the step's last key to attend
    const int pin = (int)(p - kb < DEC_BLOCK - 1 ? p - kb : DEC_BLOCK - 1);        // the row's last key, if it lies in the step
    const int lin = (int)(lo > kb ? lo - kb : 0);  // the row's first key, if it lies in the step (first - kb too: kb >= k0); <= rem, pin
    v4i kr[2][SG], vr[2][SG];
    qqq_f4 ksc[2], vsc[2];  // scales of keys kb + 16t + 4qd + r
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      // a half's addresses are a scalar base (its block's row of this KV head) plus 32-bit lane offsets inside the block
      const int8_t* kblk = k_pool + brow[t] * D;
      const int8_t* vblk = v_pool + brow[t] * D;
      const float* ksb = k_scale + brow[t];
      const float* vsb = v_scale + brow[t];
      int key = 16 * t + c < pin ? 16 * t + c : pin;  // rows outside [lo, p] load a key of the window; their scores are masked below
      key = key > lin ? key : lin;
      const int off = ((kin + key) & bmask) * D + 16 * qd;
#pragma unroll
      for (int g = 0; g < SG; ++g) {
        kr[t][g] = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(kblk + off + 64 * g));
        vr[t][g] = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(vblk + off + 64 * g));
      }
      const int g0 = 16 * t + 4 * qd;
      if (vec_scales && lin == 0) {
        const int gg = g0 < (pin & ~3) ? g0 : (pin & ~3);  // a clamped group holds masked keys only
        ksc[t] = *reinterpret_cast<const qqq_f4*>(ksb + ((kin + gg) & bmask));
        vsc[t] = *reinterpret_cast<const qqq_f4*>(vsb + ((kin + gg) & bmask));
      } else {  // also the step that holds lo (wave-uniform): no scale below lo is loaded, aligned group or not
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int kk = g0 + r < pin ? g0 + r : pin;
          kk = kk > lin ? kk : lin;
          ksc[t][r] = ksb[(kin + kk) & bmask];
          vsc[t][r] = vsb[(kin + kk) & bmask];
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
        const bool valid = 4 * qd <= rem - (16 * t + r) && 4 * qd >= lin - (16 * t + r);  // one lane value against wave-uniform ones
        const float sv = valid ? st[t][r] * (ksc[t][r] * scale_log2) : -INFINITY;
        st[t][r] = sv;
        vsc[t][r] = valid ? vsc[t][r] : 0.f;  // whatever an unwritten slot holds stays out of the product with P = 0
        mx = fmaxf(mx, sv);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);  // finite: every step that is walked holds a key of [first, last]
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
        // byte selection matrix of tile tl, made from a lane-group index the compiler cannot see through (qqq_paged_kv8_decode_split_kernel)
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
  // (Q^T in the space of lds_o: qqq_window_write_partial has a barrier between its first LDS write, to lds_m, and its writes to lds_o)
  const size_t part0 = ((size_t)bi * h + (size_t)kh * G) * splits + sp;  // partial (query 0 of kh, split sp); query g adds g * splits
  qqq_window_write_partial<D>(lds_o, lds_m, lds_l, acc, m, l, w, G, part0, splits, ws_o, ws_ml);
}

// One workgroup per batch row: merge the splits the row's placement filled -- 0 ... (pos - base) / chunk -- of all h heads, round to fp16
// once, optionally store the fp16 row, quantise it.  qqq_decode_combine_row counts its splits as p / chunk + 1, so it takes p - base.
template <int VPT, int NT>
__global__ __launch_bounds__(NT) void qqq_window_decode_combine_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                                                       const long long* __restrict__ pos, const long long limit,
                                                                       const int window, _Float16* __restrict__ o16, int8_t* __restrict__ xq,
                                                                       float* __restrict__ s1, const int h, const int d, const int chunk,
                                                                       const int splits) {
  __shared__ float red_max[NT / 64];
  const int bi = blockIdx.x;
  const long long p = pos[bi];
  if (p < 0 || p >= limit) return;  // out-of-range row: no fp16 row, no xq, no s1
  const long long base = qqq_window_lo(p, window) & ~(long long)(DEC_ROUND - 1);
  qqq_decode_combine_row<VPT, NT>(ws_o, ws_ml, bi, p - base, o16, xq, s1, h, d, chunk, splits, red_max);
}

template <int D, bool KV8>
__global__ __launch_bounds__(PF_NT) __attribute__((amdgpu_waves_per_eu(2))) void qqq_window_prefill_attn_kernel(
    const _Float16* __restrict__ q, const void* __restrict__ k_pool_v, const void* __restrict__ v_pool_v, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, const int* __restrict__ block_table, const int table_stride, const int* __restrict__ cu_tokens,
    const long long* __restrict__ start_pos, const long long limit, const int window, const float scale_log2, _Float16* __restrict__ o16,
    const int m, const int b, const int h, const int kvh, const int num_blocks, const int lbs, const int nslots) {
  constexpr int KS = D / 32;                  // k-steps of S^T = K Q^T
  constexpr int NT16 = D / 16;                // 16-column tiles of O^T
  constexpr int KLD = D + 8, VLD = D + 16;    // LDS row strides in elements: 2D + 16 and 2D + 32 bytes
  constexpr int EB = KV8 ? 1 : 2;             // bytes of a pool element
  constexpr int CPR = D * EB / 16;            // 16-byte chunks of a pool row
  constexpr int RPP = PF_NT / CPR;            // rows the workgroup loads per pass
  constexpr int NCH = PF_KT / RPP;            // passes = chunks per thread and pool
  static_assert(64 / CPR <= 16 && 16 % (64 / CPR) == 0, "a wave's rows of one pass lie in one 16-key group");
  __shared__ __attribute__((aligned(16))) _Float16 lds_k[PF_KT * KLD];
  __shared__ __attribute__((aligned(16))) _Float16 lds_v[PF_KT * VLD];
  __shared__ __attribute__((aligned(16))) float lds_ks[KV8 ? PF_KT : 4];

  const int G = h / kvh;
  const int TQ = PF_ROWS / G;  // tokens of a tile
  const int kh = blockIdx.y;
  const long long slot = (long long)nslots - 1 - blockIdx.x;
  const int si = qqq_prefill_find_seq(cu_tokens, b, m, TQ, slot);
  if (si < 0) return;
  int cu0 = cu_tokens[si], cu1 = cu_tokens[si + 1];
  cu0 = cu0 < 0 ? 0 : (cu0 > m ? m : cu0);
  cu1 = cu1 < 0 ? 0 : (cu1 > m ? m : cu1);
  const int cnt = cu1 - cu0;
  const int tile = (int)(slot - ((long long)(cu0 / TQ) + si));
  if (cnt <= 0 || (long long)tile * TQ >= cnt) return;  // a surplus slot
  const long long sp = start_pos[si];
  if (sp < 0 || sp + cnt > limit) return;  // the sequence does not fit: nothing of it is written
  const int tok0 = tile * TQ;              // first token of the tile, inside the chunk
  const int ntok = cnt - tok0 < TQ ? cnt - tok0 : TQ;
  const int start = (int)sp;
  const int last = start + tok0 + ntok - 1;                      // the tile's last key: nothing beyond it is loaded
  const int tlo = (int)qqq_window_lo(start + tok0, window);      // the tile's first key: nothing below it is loaded
  const long long kb0 = tlo & ~(PF_KT - 1);                      // the 64-key tile that holds it: the walk starts there

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, qd = lane >> 4;
  const int* table = block_table + (size_t)si * table_stride;
  const int bmask = (1 << lbs) - 1;

  // this lane's two query rows (column c of the wave's operands u = 0, 1); a row beyond the tile's tokens repeats the last one, unwritten
  int pos[2], plo[2];
  bool live[2];
  size_t orow[2];
  h8 qf[2][KS];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = 32 * w + 16 * u + c;
    int tk = row / G;
    const int g = row - tk * G;
    live[u] = tk < ntok;
    tk = tk < ntok ? tk : ntok - 1;
    pos[u] = start + tok0 + tk;
    plo[u] = (int)qqq_window_lo(pos[u], window);
    orow[u] = ((size_t)(cu0 + tok0 + tk) * h + (size_t)kh * G + g) * D;
    const _Float16* qr = q + orow[u] + 8 * qd;
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[u][s] = *reinterpret_cast<const h8*>(qr + 32 * s);
  }
  // the wave's first and last positions (rows are in token order) and the first keys of their bands: steps beyond the last position or
  // below the first band are skipped, steps from the last band up to the first position need no mask
  int t_lo = (32 * w) / G, t_hi = (32 * w + 31) / G;
  t_lo = t_lo < ntok ? t_lo : ntok - 1;
  t_hi = t_hi < ntok ? t_hi : ntok - 1;
  const int wpos_lo = start + tok0 + t_lo, wpos_hi = start + tok0 + t_hi;
  const int wlo_lo = (int)qqq_window_lo(wpos_lo, window), wlo_hi = (int)qqq_window_lo(wpos_hi, window);

  qqq_f4 acc[2][NT16];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int n = 0; n < NT16; ++n) acc[u][n] = qqq_f4{0.f, 0.f, 0.f, 0.f};
  float mrun[2] = {-INFINITY, -INFINITY}, lrun[2] = {0.f, 0.f};

  // staging: chunk (row0 + RPP i, col) of the tile, i < NCH
  const int srow0 = tid / CPR, scol = tid - srow0 * CPR;
  v4i kreg[NCH], vreg[NCH];
  float ksreg[KV8 ? NCH : 1], vsreg[KV8 ? NCH : 1];
  int bid[NCH];  // block ids of the groups this wave loads from in the next tile to load
  const char* kp = static_cast<const char*>(k_pool_v);
  const char* vp = static_cast<const char*>(v_pool_v);

  auto fetch_ids = [&](const long long kb) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      long long gk = kb + ((w * (64 / CPR) + RPP * i) & ~15);  // first key of the 16-key group of this wave's rows in pass i
      gk = gk < last ? gk : last;
      gk = gk > tlo ? gk : tlo;  // a group that starts below the tile's first key loads that key's block: the clamp of load_tile
      int blk = table[__builtin_amdgcn_readfirstlane((int)(gk >> lbs))];
      bid[i] = blk < 0 ? 0 : (blk >= num_blocks ? num_blocks - 1 : blk);
    }
  };
  auto load_tile = [&](const long long kb) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const long long kk = kb + srow0 + RPP * i;
      int key = (int)(kk < last ? kk : last);  // a key outside [tlo, last] is never loaded; its score is masked
      key = key > tlo ? key : tlo;
      const size_t prow = (((size_t)bid[i] * kvh + kh) << lbs) + (size_t)(key & bmask);
      kreg[i] = *reinterpret_cast<const v4i*>(kp + (prow * D) * EB + 16 * scol);
      vreg[i] = *reinterpret_cast<const v4i*>(vp + (prow * D) * EB + 16 * scol);
      if (KV8) {
        ksreg[i] = k_scale[prow];
        vsreg[i] = v_scale[prow];
      }
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int row = srow0 + RPP * i;
      if (KV8) {
        _Float16* kd = lds_k + row * KLD + 16 * scol;
        _Float16* vd = lds_v + row * VLD + 16 * scol;
        *reinterpret_cast<h8*>(kd) = qqq_kv8_codes_to_h8(kreg[i][0], kreg[i][1]);
        *reinterpret_cast<h8*>(kd + 8) = qqq_kv8_codes_to_h8(kreg[i][2], kreg[i][3]);
        h8 x[2];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int code = (int)(signed char)(((unsigned)vreg[i][e >> 2] >> (8 * (e & 3))) & 0xffu);
          x[e >> 3][e & 7] = (_Float16)((float)code * vsreg[i]);
        }
        *reinterpret_cast<h8*>(vd) = x[0];
        *reinterpret_cast<h8*>(vd + 8) = x[1];
        if (scol == 0) lds_ks[row] = ksreg[i];
      } else {
        *reinterpret_cast<v4i*>(lds_k + row * KLD + 8 * scol) = kreg[i];
        *reinterpret_cast<v4i*>(lds_v + row * VLD + 8 * scol) = vreg[i];
      }
    }
  };

  fetch_ids(kb0);
  load_tile(kb0);
  fetch_ids(kb0 + PF_KT);
  for (long long kb = kb0; kb <= last; kb += PF_KT) {  // 64-bit: last may be close to 2^31
    __syncthreads();  // the previous tile has been read
    store_tile();
    __syncthreads();
    if (kb + PF_KT <= last) {
      load_tile(kb + PF_KT);
      fetch_ids(kb + 2 * PF_KT);
    }
#pragma unroll
    for (int ss = 0; ss < PF_KT / 32; ++ss) {
      const long long k0 = kb + 32 * ss;
      if (k0 > wpos_hi) break;          // wholly above the diagonal for every row of this wave (wave-uniform)
      if (k0 + 31 < wlo_lo) continue;   // wholly below the band of every row of this wave (wave-uniform)
      const bool diag = k0 + 31 > wpos_lo, edge = k0 < wlo_hi;
      int rel[2], rlo[2];  // the last and the first key of the step each row attends, relative to k0
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        rel[u] = (int)(pos[u] - k0 < 32 ? pos[u] - k0 : 32);
        rlo[u] = (int)(plo[u] - k0 > 0 ? plo[u] - k0 : 0);
      }
      qqq_f4 st[2][2];  // S^T: operand u, half t: lane l, register r = score of query c against key k0 + 16t + 4qd + r
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const _Float16* kr = lds_k + (32 * ss + 16 * t + c) * KLD + 8 * qd;
        h8 kf[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) kf[s] = *reinterpret_cast<const h8*>(kr + 32 * s);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          st[u][t] = qqq_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KS; ++s) st[u][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[s], qf[u][s], st[u][t], 0, 0, 0);
        }
      }
      qqq_f4 ksc[2];
      if (KV8) {
#pragma unroll
        for (int t = 0; t < 2; ++t) ksc[t] = *reinterpret_cast<const qqq_f4*>(lds_ks + 32 * ss + 16 * t + 4 * qd) * scale_log2;
      }
      h8 pf[2];  // B operands of O^T: P[query c][key k0 + 16 (j >> 2) + 4qd + (j & 3)] in fp16
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float sv = KV8 ? st[u][t][r] * ksc[t][r] : st[u][t][r] * scale_log2;
            if (diag) sv = (16 * t + 4 * qd + r <= rel[u]) ? sv : -INFINITY;
            if (edge) sv = (16 * t + 4 * qd + r >= rlo[u]) ? sv : -INFINITY;
            st[u][t][r] = sv;
            mx = fmaxf(mx, sv);
          }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(mrun[u], mx);  // -inf while the row has met no key of its band: the step is then an exact no-op
        const float ms = mn == -INFINITY ? 0.f : mn;
        const float alpha = exp2f(mrun[u] - ms);
        mrun[u] = mn;
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const _Float16 ph = (_Float16)exp2f(st[u][t][r] - ms);
            pf[u][4 * t + r] = ph;
            ps += (float)ph;
          }
        lrun[u] = lrun[u] * alpha + ps;
#pragma unroll
        for (int n = 0; n < NT16; ++n) acc[u][n] *= alpha;
      }
      // V^T rows d = 16n + c of keys k0 + 16t + 4qd + r, in the key order of pf: two transposed reads per 16-column tile
      const _Float16* vr = lds_v + (32 * ss + 4 * qd + (c >> 2)) * VLD + 4 * (c & 3);
#pragma unroll
      for (int n = 0; n < NT16; ++n) {
        const qqq_s4 v0 = qqq_prefill_tr_read(vr + 16 * n), v1 = qqq_prefill_tr_read(vr + 16 * VLD + 16 * n);
        typedef short qqq_s8 __attribute__((ext_vector_type(8)));
        const qqq_s8 vs = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        const h8 va = __builtin_bit_cast(h8, vs);
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[u][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pf[u], acc[u][n], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    float l = lrun[u];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (live[u]) {
      _Float16* orp = o16 + orow[u] + 4 * qd;
#pragma unroll
      for (int n = 0; n < NT16; ++n) {
        const h4 x = {(_Float16)(acc[u][n][0] / l), (_Float16)(acc[u][n][1] / l), (_Float16)(acc[u][n][2] / l),
                      (_Float16)(acc[u][n][3] / l)};
        *reinterpret_cast<h4*>(orp + 16 * n) = x;
      }
    }
  }
}

#endif  // QQQ_AMD_QQQ_WINDOW_HIP_H_
