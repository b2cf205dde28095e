// qqq_paged.hip.h -- the block-table (paged) KV cache (include/qqq_amd_paged.h): the RoPE / cache-write kernels that put every token's k / v
// row at a slot of a block pool, and the split kernels of the decode attention that read a row's keys through its block table.  Part of the
// single translation unit qqq_w4a8.hip.
//
// Pools: k_pool / v_pool [num_blocks, kvh, block_size, d] (fp16 or int8), an int8 pool with k_scale / v_scale [num_blocks, kvh, block_size].
// Inside a (block, KV head) the layout is the contiguous caches' [key][d], so the 16-byte K / V loads, the scale vectors and the MFMA
// dataflow of qqq_decode_split_kernel / qqq_kv8_decode_split_kernel carry over unchanged; only the addresses differ.
//
//   qqq_paged_rope_qkv_kernel        qqq_rope_qkv_kernel's items and arithmetic (qqq_rope_half); the k / v row of token t goes to slot
//   qqq_paged_kv8_rope_qkv_kernel    slots[t] = block * block_size + offset, q_out is token-major [m, h, d].  The int8 variant quantises
//                                    every cached row with qqq_kv8_quant_head_row.  A slot outside the pool writes q_out only.
//   qqq_paged_decode_split_kernel    the contiguous split kernels with key j of row bi in block block_table[bi * table_stride + (j >> lbs)]
//   qqq_paged_kv8_decode_split_kernel  at slot j & (block_size - 1).  block_size >= 16 is a power of two and a wave's 32-key step starts at a
//                                    multiple of 32, so each 16-key half of a step lies in one block: its id is one wave-uniform (scalar) table
//                                    load per half and step -- one per step where block_size >= 32 -- fetched one step ahead, clamped into
//                                    [0, num_blocks).  A half that starts beyond the row's last key p takes p's block: every key a lane loads
//                                    is min(key, p), so only table entries 0 ... p / block_size are read.  Same grid, chunking, online
//                                    softmax, LDS merge and workspace layout, and the same order of every sum: the partials are bit for bit
//                                    the contiguous kernels', and qqq_decode_combine_kernel finishes the call unchanged.
#ifndef QQQ_AMD_QQQ_PAGED_HIP_H_
#define QQQ_AMD_QQQ_PAGED_HIP_H_

// the first row ([key 0][d]) of (block holding key `key`, KV head kh), in rows of the pool; `key` is wave-uniform
__device__ __forceinline__ size_t qqq_paged_block_row(const int* __restrict__ table, const long long key, const int lbs, const int num_blocks,
                                                      const int kvh, const int kh) {
  int blk = table[__builtin_amdgcn_readfirstlane((int)(key >> lbs))];
  blk = blk < 0 ? 0 : (blk >= num_blocks ? num_blocks - 1 : blk);  // a corrupt table gives a wrong row, never an address outside the pool
  return ((size_t)blk * kvh + kh) << lbs;
}

template <int NT>
__global__ __launch_bounds__(NT) void qqq_paged_rope_qkv_kernel(const _Float16* __restrict__ q, const int ld_q, const _Float16* __restrict__ k,
                                                                const int ld_k, const _Float16* __restrict__ v, const int ld_v,
                                                                const _Float16* __restrict__ cos_t, const _Float16* __restrict__ sin_t,
                                                                const long long* __restrict__ pos, const long long limit,
                                                                const long long* __restrict__ slots, const long long nslots,
                                                                _Float16* __restrict__ q_out, _Float16* __restrict__ k_pool,
                                                                _Float16* __restrict__ v_pool, const int h, const int kvh, const int d,
                                                                const int lbs) {
  const int t = blockIdx.x;  // token
  const long long p = pos[t];
  if (p < 0 || p >= limit) return;  // nothing of this token is written
  const int P = d >> 4;             // items per head
  const int item = blockIdx.y * NT + threadIdx.x;
  if (item >= (h + 2 * kvh) * P) return;
  const int hd = d >> 1;
  int head = item / P;
  const int j = (item - head * P) * 8;  // element offset of this lane's vector in the first half-head
  const long long slot = slots[t];
  if (head >= h && (slot < 0 || slot >= nslots)) return;  // a padding slot: the token's q_out row only
  const size_t blk = (size_t)(slot >> lbs), in_blk = (size_t)(slot & ((1 << lbs) - 1));
  const _Float16* src;
  _Float16* dst;
  if (head < h) {
    src = q + (size_t)t * ld_q + (size_t)head * d;
    dst = q_out + ((size_t)t * h + head) * d;
  } else if (head < h + kvh) {
    head -= h;
    src = k + (size_t)t * ld_k + (size_t)head * d;
    dst = k_pool + ((((blk * kvh + head) << lbs) + in_blk)) * d;
  } else {
    head -= h + kvh;
    const h8* vs = reinterpret_cast<const h8*>(v + (size_t)t * ld_v + (size_t)head * d + j);
    h8* vd = reinterpret_cast<h8*>(v_pool + ((((blk * kvh + head) << lbs) + in_blk)) * d + j);
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

template <int NT>
__global__ __launch_bounds__(NT) void qqq_paged_kv8_rope_qkv_kernel(
    const _Float16* __restrict__ q, const int ld_q, const _Float16* __restrict__ k, const int ld_k, const _Float16* __restrict__ v,
    const int ld_v, const _Float16* __restrict__ cos_t, const _Float16* __restrict__ sin_t, const long long* __restrict__ pos,
    const long long limit, const long long* __restrict__ slots, const long long nslots, _Float16* __restrict__ q_out,
    int8_t* __restrict__ k_pool, int8_t* __restrict__ v_pool, float* __restrict__ k_scale, float* __restrict__ v_scale, const int h,
    const int kvh, const int d, const int lbs) {
  const int t = blockIdx.x;  // token
  const long long p = pos[t];
  if (p < 0 || p >= limit) return;  // nothing of this token is written
  const int P = d >> 4;             // items per head: 4 or 8, so a head's lanes are neighbours in one wave
  const int item = blockIdx.y * NT + threadIdx.x;
  if (item >= (h + 2 * kvh) * P) return;  // whole heads: (h + 2 kvh) P is a multiple of P
  const int hd = d >> 1;
  int head = item / P;
  const int j = (item - head * P) * 8;  // element offset of this lane's vector in the first half-head
  const long long slot = slots[t];
  if (head >= h && (slot < 0 || slot >= nslots)) return;  // a padding slot: the token's q_out row only (whole heads leave together)
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
    _Float16* dst = q_out + ((size_t)t * h + head) * d;
    *reinterpret_cast<h8*>(dst + j) = lo;
    *reinterpret_cast<h8*>(dst + hd + j) = hi;
    return;
  }
  const bool is_v = head >= h + kvh;
  head -= is_v ? h + kvh : h;
  const size_t row = ((((size_t)(slot >> lbs) * kvh + head) << lbs) + (size_t)(slot & ((1 << lbs) - 1)));
  qqq_kv8_quant_head_row(lo, hi, P, j, hd, (is_v ? v_pool : k_pool) + row * d, (is_v ? v_scale : k_scale) + row);
}

template <int D>
__global__ __launch_bounds__(DEC_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void qqq_paged_decode_split_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ k_pool, const _Float16* __restrict__ v_pool,
    const int* __restrict__ block_table, const int table_stride, const long long* __restrict__ pos, const long long limit,
    const float scale_log2, float* __restrict__ ws_o, float* __restrict__ ws_ml, const int h, const int kvh, const int num_blocks,
    const int lbs, const int chunk, const int splits) {
  constexpr int KS = D / 32;    // k-steps of S^T = K Q^T
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

  // block rows of the two 16-key halves of a step, fetched one step ahead.  A half that starts beyond p takes p's block.
  long long kb = k0 + (long long)DEC_BLOCK * w;
  size_t nrow[2] = {0, 0};
  if (kb <= last) {
    nrow[0] = qqq_paged_block_row(table, kb, lbs, num_blocks, kvh, kh);
    nrow[1] = lbs >= 5 ? nrow[0] : qqq_paged_block_row(table, kb + 16 < p ? kb + 16 : p, lbs, num_blocks, kvh, kh);
  }
  for (; kb <= last; kb += DEC_ROUND) {
    const size_t brow[2] = {nrow[0], nrow[1]};
    const long long nk = kb + DEC_ROUND;
    if (nk <= last) {
      nrow[0] = qqq_paged_block_row(table, nk, lbs, num_blocks, kvh, kh);
      nrow[1] = lbs >= 5 ? nrow[0] : qqq_paged_block_row(table, nk + 16 < p ? nk + 16 : p, lbs, num_blocks, kvh, kh);
    }
    h8 kf[2][KS], vf[2][KS];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      long long key = kb + 16 * t + c;
      key = key > p ? p : key;  // rows past the last key load a valid row; their scores are masked below
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

template <int D>
__global__ __launch_bounds__(DEC_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void qqq_paged_kv8_decode_split_kernel(
    const _Float16* __restrict__ q, const int8_t* __restrict__ k_pool, const int8_t* __restrict__ v_pool, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, const int* __restrict__ block_table, const int table_stride, const long long* __restrict__ pos,
    const long long limit, const float scale_log2, float* __restrict__ ws_o, float* __restrict__ ws_ml, const int h, const int kvh,
    const int num_blocks, const int lbs, const int chunk, const int splits) {
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
  const int* table = block_table + (size_t)bi * table_stride;
  const int bmask = (1 << lbs) - 1;

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
  // 16-byte scale loads need the scale pools 16-byte aligned: a (block, head) row of scales is block_size >= 16 floats long
  const bool vec_scales = (((uintptr_t)k_scale | (uintptr_t)v_scale) & 15) == 0;

  // block rows of the two 16-key halves of a step, fetched one step ahead.  A half that starts beyond p takes p's block.
  long long kb = k0 + (long long)DEC_BLOCK * w;
  size_t nrow[2] = {0, 0};
  if (kb <= last) {
    nrow[0] = qqq_paged_block_row(table, kb, lbs, num_blocks, kvh, kh);
    nrow[1] = lbs >= 5 ? nrow[0] : qqq_paged_block_row(table, kb + 16 < p ? kb + 16 : p, lbs, num_blocks, kvh, kh);
  }
  for (; kb <= last; kb += DEC_ROUND) {
    const size_t brow[2] = {nrow[0], nrow[1]};
    const long long nk = kb + DEC_ROUND;
    if (nk <= last) {
      nrow[0] = qqq_paged_block_row(table, nk, lbs, num_blocks, kvh, kh);
      nrow[1] = lbs >= 5 ? nrow[0] : qqq_paged_block_row(table, nk + 16 < p ? nk + 16 : p, lbs, num_blocks, kvh, kh);
    }
    const int kin = (int)kb & bmask;  // the step's first key inside its block (0 where block_size is 16 or 32)
    const int rem = (int)(last - kb < DEC_BLOCK - 1 ? last - kb : DEC_BLOCK - 1);  // the block's last key to attend
    const int pin = (int)(p - kb < DEC_BLOCK - 1 ? p - kb : DEC_BLOCK - 1);        // the row's last key, if it lies in the block
    v4i kr[2][SG], vr[2][SG];
    qqq_f4 ksc[2], vsc[2];  // scales of keys kb + 16t + 4qd + r
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      // a half's addresses are a scalar base (its block's row of this KV head) plus 32-bit lane offsets inside the block
      const int8_t* kblk = k_pool + brow[t] * D;
      const int8_t* vblk = v_pool + brow[t] * D;
      const float* ksb = k_scale + brow[t];
      const float* vsb = v_scale + brow[t];
      const int key = 16 * t + c < pin ? 16 * t + c : pin;  // rows past the row's last key load that key; their scores are masked below
      const int off = ((kin + key) & bmask) * D + 16 * qd;
#pragma unroll
      for (int g = 0; g < SG; ++g) {
        kr[t][g] = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(kblk + off + 64 * g));
        vr[t][g] = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(vblk + off + 64 * g));
      }
      const int g0 = 16 * t + 4 * qd;
      if (vec_scales) {
        const int gg = g0 < (pin & ~3) ? g0 : (pin & ~3);  // a clamped group holds masked keys only
        ksc[t] = *reinterpret_cast<const qqq_f4*>(ksb + ((kin + gg) & bmask));
        vsc[t] = *reinterpret_cast<const qqq_f4*>(vsb + ((kin + gg) & bmask));
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kk = g0 + r < pin ? g0 + r : pin;
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

#endif  // QQQ_AMD_QQQ_PAGED_HIP_H_
