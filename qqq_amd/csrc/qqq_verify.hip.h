// qqq_verify.hip.h -- split-K attention of a verify chunk: T = draft_len + 1 consecutive tokens per batch row over the block-table KV cache
// (include/qqq_amd_verify.h), every token's output produced already int8-quantised for o_proj.  Part of the single translation unit
// qqq_w4a8.hip.
//
// qqq_paged_decode_split_kernel pads the G = h / kvh query heads of a KV head to the 16 query rows of an MFMA tile.  A verify chunk's
// G * T rows go into that padding, and into up to three further tiles: query row t * G + g of batch row r is token t (position
// start[r] + t), query head g.  Rows beyond G * T hold q = 0 and are never stored.
//
//   qqq_verify_split_kernel            grid (splits, kvh, b), 4 waves, templated on D and on the number NQ of 16-row query tiles.  Chunking
//   qqq_verify_kv8_split_kernel        is decode_split_plan(dev, b, kvh, max_len) -- b the batch rows, not the tokens.  A wave walks the
//                                      32-key blocks w, w + 4, ... of its chunk up to the last key ANY token of the row may see,
//                                      min(k0 + chunk - 1, start + T - 1, max_len - 1); every loaded key is the minimum of itself and that
//                                      key, so only table entries 0 ... (start + T - 1) / block_size are read.  The K and V fragments of a
//                                      block and the two selection MFMAs per V fragment are issued once and shared by the NQ tiles; a tile
//                                      adds its own S and PV MFMAs.  Q^T waits in LDS (in the space of the merge buffer).
//   causal limit                       the score of key j for token t is -inf where j > start + t.  The online-softmax statistics are per
//                                      query row, so a block wholly beyond a row's limit is an exact no-op for it: alpha = 1, P = 0, l and
//                                      the accumulator unchanged (0 * a finite V adds nothing).  A row that has seen no key yet has
//                                      m = -inf as well as mx = -inf; the -inf - (-inf) of that case is guarded (it cannot occur in the
//                                      decode kernel, whose loop ends at pos; here it occurs in every row but the last).
//   wave merge                         the decode kernel's, one 16-row tile per pass through a merge buffer of 4 x 16 x D floats, and its
//                                      partial layout with token row (r * T + t) * h + head in place of bi * h + head.  A split that
//                                      starts beyond token t's position writes no partial for it.
//   qqq_verify_combine_kernel          grid (b * T): qqq_decode_combine_row (qqq_decode.hip.h) with p = start[r] + t.  Token t of row r
//                                      writes nothing if start[r] < 0 or start[r] + t >= max_len.
//
// The blocks a token's row takes part in, the masks inside them and the order of every sum are those of the decode kernels for that token
// alone (pos = start + t, equal b, kvh and max_len), and an MFMA column does not see its neighbours: o_fp16, xq and s1 of every token
// are bit for bit qqq_decode_attn_paged(_kv8)'s.
//
// Registers: a tile keeps D / 4 accumulator registers, so NQ = 4 at D = 128 holds 128 of them beside the 64 of a block's fp16 K and V
// fragments: that instantiation runs one wave per SIMD (the 512-register budget), NQ = 2 two, NQ = 1 the decode kernel's four -- three
// over an int8 pool at D = 128, where the per-row limits beside the decode kernel's 126 registers would put four in scratch.  No
// instantiation uses scratch.
#ifndef QQQ_AMD_QQQ_VERIFY_HIP_H_
#define QQQ_AMD_QQQ_VERIFY_HIP_H_

static constexpr int VER_TMAX = 16;     // tokens of a chunk
static constexpr int VER_ROWS_MAX = 64;  // query rows (G * T) of a KV head: four tiles

// waves per SIMD of an instantiation (see above)
constexpr int qqq_verify_waves(const int D, const int NQ, const bool kv8) {
  return NQ == 1 ? (kv8 && D == 128 ? 3 : 4) : (NQ == 2 ? 2 : (D == 128 ? 1 : 2));
}

// Q^T of the chunk into LDS: query row R = t * G + g of ROWS (zeros from G * T on), rows QLD elements apart
template <int D, int ROWS, int QLD>
__device__ __forceinline__ void qqq_verify_stage_q(_Float16* lds_q, const _Float16* __restrict__ q, const int bi, const int kh, const int h,
                                                   const int G, const int T) {
  for (int i = threadIdx.x; i < ROWS * (D / 8); i += DEC_WAVES * 64) {
    const int row = i / (D / 8), e = (i - row * (D / 8)) * 8;
    const int tok = row / G, g = row - tok * G;
    h8 x = h8{};
    if (tok < T) x = *reinterpret_cast<const h8*>(q + (((size_t)bi * T + tok) * h + (size_t)kh * G + g) * D + e);
    *reinterpret_cast<h8*>(lds_q + row * QLD + e) = x;
  }
}

// The merge of the four waves and the partials of the chunk's tokens: qqq_paged_decode_split_kernel's, tile by tile.  lds_o is free of Q^T
// once every wave has left its loop (the first barrier below).  rel0 = start - k0: token tok takes part in this split iff rel0 + tok >= 0.
template <int D, int NQ>
__device__ __forceinline__ void qqq_verify_merge(float (&lds_o)[DEC_WAVES][16][D], float (&lds_m)[DEC_WAVES][16 * NQ],
                                                 float (&lds_l)[DEC_WAVES][16 * NQ], const qqq_f4 (&acc)[NQ][D / 16], const float (&m)[NQ],
                                                 const float (&l)[NQ], const int w, const int tid, const int bi, const int kh, const int sp,
                                                 const int h, const int G, const int T, const long long rel0, const int splits,
                                                 float* __restrict__ ws_o, float* __restrict__ ws_ml) {
  constexpr int NT16 = D / 16;
  const int ce = tid & 15, qe = (tid >> 4) & 3;
  const int nrows = G * T;
  if (qe == 0) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      lds_m[w][16 * i + ce] = m[i];
      lds_l[w][16 * i + ce] = l[i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    if (16 * i < nrows) {  // workgroup-uniform: a tile of padding alone has nothing to merge
      {
        float M = lds_m[0][16 * i + ce];
#pragma unroll
        for (int ww = 1; ww < DEC_WAVES; ++ww) M = fmaxf(M, lds_m[ww][16 * i + ce]);
        const float f = exp2f(m[i] - M);  // a wave without a block for this row has m = -inf and f = 0; M = -inf only in rows not stored
#pragma unroll
        for (int n = 0; n < NT16; ++n) *reinterpret_cast<qqq_f4*>(&lds_o[w][ce][16 * n + 4 * qe]) = acc[i][n] * f;
      }
      __syncthreads();
      for (int j = tid; j < 16 * (D / 4); j += DEC_WAVES * 64) {
        const int rr = j / (D / 4), e = (j - rr * (D / 4)) * 4;
        const int row = 16 * i + rr;
        const int tok = row / G, g = row - tok * G;
        if (row >= nrows || rel0 + tok < 0) continue;  // padding, or the split starts beyond this token's position
        qqq_f4 o = *reinterpret_cast<const qqq_f4*>(&lds_o[0][rr][e]);
#pragma unroll
        for (int ww = 1; ww < DEC_WAVES; ++ww) o += *reinterpret_cast<const qqq_f4*>(&lds_o[ww][rr][e]);
        const size_t part = (((size_t)bi * T + tok) * h + (size_t)kh * G + g) * splits + sp;
        *reinterpret_cast<qqq_f4*>(ws_o + part * D + e) = o;
      }
      __syncthreads();
    }
  }
  if (tid < nrows) {
    const int tok = tid / G, g = tid - tok * G;
    if (rel0 + tok >= 0) {
      float M = lds_m[0][tid];
#pragma unroll
      for (int ww = 1; ww < DEC_WAVES; ++ww) M = fmaxf(M, lds_m[ww][tid]);
      float L = 0.f;
#pragma unroll
      for (int ww = 0; ww < DEC_WAVES; ++ww) L += lds_l[ww][tid] * exp2f(lds_m[ww][tid] - M);
      const size_t part = (((size_t)bi * T + tok) * h + (size_t)kh * G + g) * splits + sp;
      reinterpret_cast<float2*>(ws_ml)[part] = make_float2(M, L);
    }
  }
}

template <int D, int NQ>
__global__ __launch_bounds__(DEC_WAVES * 64) __attribute__((amdgpu_waves_per_eu(qqq_verify_waves(D, NQ, false)))) void qqq_verify_split_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ k_pool, const _Float16* __restrict__ v_pool,
    const int* __restrict__ block_table, const int table_stride, const long long* __restrict__ start, const long long limit,
    const float scale_log2, float* __restrict__ ws_o, float* __restrict__ ws_ml, const int h, const int kvh, const int T,
    const int num_blocks, const int lbs, const int chunk, const int splits) {
  constexpr int KS = D / 32;    // k-steps of S^T = K Q^T
  constexpr int NT16 = D / 16;  // 16-column tiles of O^T
  constexpr int ROWS = 16 * NQ, QLD = D + 8;
  __shared__ float lds_o[DEC_WAVES][16][D];
  __shared__ float lds_m[DEC_WAVES][ROWS], lds_l[DEC_WAVES][ROWS];
  static_assert(ROWS * QLD * sizeof(_Float16) <= sizeof(lds_o), "Q^T waits in the merge buffer");
  const int sp = blockIdx.x, kh = blockIdx.y, bi = blockIdx.z;
  const long long p0 = start[bi];
  if (p0 < 0 || p0 >= limit) return;  // no token of the row is in range: nothing is written
  const long long p = p0 + T - 1 < limit - 1 ? p0 + T - 1 : limit - 1;  // the last key any token of the row may see
  const long long k0 = (long long)sp * chunk;
  if (k0 > p) return;  // the split lies wholly beyond the row's last key
  const long long last = (k0 + chunk - 1 < p) ? k0 + chunk - 1 : p;
  const int G = h / kvh;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform and known to be: the table loads are scalar
  const int c = lane & 15, qd = lane >> 4;
  const int* table = block_table + (size_t)bi * table_stride;
  const int bmask = (1 << lbs) - 1;

  _Float16* lds_q = reinterpret_cast<_Float16*>(&lds_o[0][0][0]);
  qqq_verify_stage_q<D, ROWS, QLD>(lds_q, q, bi, kh, h, G, T);
  __syncthreads();
  const _Float16* qrow = lds_q + c * QLD + 8 * qd;  // B operand of S^T: query row 16i + c, head elements 32s + 8qd + j

  // the last key of query row 16i + c, counted from k0: below 0 for padding rows and for tokens this split starts beyond
  int rl[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int tok = (16 * i + c) / G;
    const long long pt = p0 + tok < last ? p0 + tok : last;
    rl[i] = tok < T ? (int)(pt - k0) : -1;
  }
  h8 sel[2];  // selection matrices: column n of half hh takes k index n + 16 hh (lane l holds k = 8qd + j of column c)
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int j = 0; j < 8; ++j) sel[hh][j] = (8 * qd + j == c + 16 * hh) ? (_Float16)1.0f : (_Float16)0.0f;

  qqq_f4 acc[NQ][NT16];  // O^T tile n of query tile i: lane l, register r = O[query 16i + c][16n + 4qd + r]
  float m[NQ], l[NQ];    // running max (log2 domain) and this lane's share of the running sum, for query row 16i + c
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
#pragma unroll
    for (int n = 0; n < NT16; ++n) acc[i][n] = qqq_f4{0.f, 0.f, 0.f, 0.f};
    m[i] = -INFINITY;
    l[i] = 0.f;
  }

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
      key = key > p ? p : key;  // rows past the row's last key load a valid row; their scores are masked below
      const int off = ((int)key & bmask) * D + 8 * qd;
      const _Float16* kblk = k_pool + brow[t] * D;
      const _Float16* vblk = v_pool + brow[t] * D;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        kf[t][s] = *reinterpret_cast<const h8*>(kblk + off + 32 * s);
        vf[t][s] = *reinterpret_cast<const h8*>(vblk + off + 32 * s);
      }
    }
    const int kr = (int)(kb - k0) + 4 * qd;  // key kb + 16t + 4qd + r, counted from k0, is kr + 16t + r
    h8 pf[NQ];  // B operand of O^T: P[query 16i + c][key kb + 16 (j >> 2) + 4qd + (j & 3)] in fp16
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      h8 qf[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const h8*>(qrow + 16 * i * QLD + 32 * s);
      qqq_f4 st[2];  // S^T: lane l, register r of half t = score of query 16i + c against key kb + 16t + 4qd + r
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        st[t] = qqq_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) st[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[t][s], qf[s], st[t], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float sv = (kr + 16 * t + r <= rl[i]) ? st[t][r] * scale_log2 : -INFINITY;
          st[t][r] = sv;
          mx = fmaxf(mx, sv);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m[i], mx);
      const bool none = mn == -INFINITY;  // the row has seen no key yet, this block included: -inf - (-inf) below
      const float alpha = none ? 1.f : exp2f(m[i] - mn);
      const float mz = none ? 0.f : mn;
      m[i] = mn;
      float ps = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const _Float16 ph = (_Float16)exp2f(st[t][r] - mz);
          pf[i][4 * t + r] = ph;
          ps += (float)ph;
        }
      l[i] = l[i] * alpha + ps;
#pragma unroll
      for (int n = 0; n < NT16; ++n) acc[i][n] *= alpha;
    }
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        // V^T rows d = 32s + 16hh + c of keys kb + 16t + 4qd + r (t = 0, 1), in the key order of pf: once for all the tiles
        const qqq_f4 z = qqq_f4{0.f, 0.f, 0.f, 0.f};
        const qqq_f4 t0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[0][s], sel[hh], z, 0, 0, 0);
        const qqq_f4 t1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[1][s], sel[hh], z, 0, 0, 0);
        const h8 va = {(_Float16)t0[0], (_Float16)t0[1], (_Float16)t0[2], (_Float16)t0[3],
                       (_Float16)t1[0], (_Float16)t1[1], (_Float16)t1[2], (_Float16)t1[3]};
#pragma unroll
        for (int i = 0; i < NQ; ++i) acc[i][2 * s + hh] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pf[i], acc[i][2 * s + hh], 0, 0, 0);
      }
  }
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    l[i] += __shfl_xor(l[i], 16);
    l[i] += __shfl_xor(l[i], 32);
  }
  // the lane indices are taken afresh, so that the addresses of the merge are worked out there and not carried through the loop
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  qqq_verify_merge<D, NQ>(lds_o, lds_m, lds_l, acc, m, l, w, tid, bi, kh, sp, h, G, T, p0 - k0, splits, ws_o, ws_ml);
}

template <int D, int NQ>
__global__ __launch_bounds__(DEC_WAVES * 64) __attribute__((amdgpu_waves_per_eu(qqq_verify_waves(D, NQ, true)))) void qqq_verify_kv8_split_kernel(
    const _Float16* __restrict__ q, const int8_t* __restrict__ k_pool, const int8_t* __restrict__ v_pool, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, const int* __restrict__ block_table, const int table_stride, const long long* __restrict__ start,
    const long long limit, const float scale_log2, float* __restrict__ ws_o, float* __restrict__ ws_ml, const int h, const int kvh,
    const int T, const int num_blocks, const int lbs, const int chunk, const int splits) {
  constexpr int SG = D / 64;    // 64-element segments of a head row: one 16-byte load per lane each
  constexpr int NT16 = D / 16;  // 16-column tiles of O^T
  constexpr int ROWS = 16 * NQ, QLD = D + 8;
  __shared__ float lds_o[DEC_WAVES][16][D];
  __shared__ float lds_m[DEC_WAVES][ROWS], lds_l[DEC_WAVES][ROWS];
  static_assert(ROWS * QLD * sizeof(_Float16) <= sizeof(lds_o), "Q^T waits in the merge buffer");
  const int sp = blockIdx.x, kh = blockIdx.y, bi = blockIdx.z;
  const long long p0 = start[bi];
  if (p0 < 0 || p0 >= limit) return;  // no token of the row is in range: nothing is written
  const long long p = p0 + T - 1 < limit - 1 ? p0 + T - 1 : limit - 1;  // the last key any token of the row may see
  const long long k0 = (long long)sp * chunk;
  if (k0 > p) return;  // the split lies wholly beyond the row's last key
  const long long last = (k0 + chunk - 1 < p) ? k0 + chunk - 1 : p;
  const int G = h / kvh;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform and known to be: a block's addresses stay in SGPRs
  const int c = lane & 15, qd = lane >> 4;
  const int* table = block_table + (size_t)bi * table_stride;
  const int bmask = (1 << lbs) - 1;

  _Float16* lds_q = reinterpret_cast<_Float16*>(&lds_o[0][0][0]);
  qqq_verify_stage_q<D, ROWS, QLD>(lds_q, q, bi, kh, h, G, T);
  __syncthreads();
  const _Float16* qrow = lds_q + c * QLD + 16 * qd;  // elements 64g + 16qd + 8u + j: the order of a K load's bytes
  v4i onehot;  // byte c of the lane's 16
#pragma unroll
  for (int i = 0; i < 4; ++i) onehot[i] = ((c >> 2) == i) ? (1 << (8 * (c & 3))) : 0;

  // the last key of query row 16i + c, counted from k0: below 0 for padding rows and for tokens this split starts beyond
  int rl[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int tok = (16 * i + c) / G;
    const long long pt = p0 + tok < last ? p0 + tok : last;
    rl[i] = tok < T ? (int)(pt - k0) : -1;
  }
  qqq_f4 acc[NQ][NT16];  // O^T tile n of query tile i: lane l, register r = O[query 16i + c][16n + 4qd + r]
  float m[NQ], l[NQ];    // running max (log2 domain) and this lane's share of the running sum, for query row 16i + c
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
#pragma unroll
    for (int n = 0; n < NT16; ++n) acc[i][n] = qqq_f4{0.f, 0.f, 0.f, 0.f};
    m[i] = -INFINITY;
    l[i] = 0.f;
  }
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
    const int rem = (int)(last - kb < DEC_BLOCK - 1 ? last - kb : DEC_BLOCK - 1);  // the block's last key any token attends
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
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool valid = 4 * qd <= rem - (16 * t + r);  // one lane value against eight wave-uniform ones
        vsc[t][r] = valid ? vsc[t][r] : 0.f;               // whatever an unwritten slot holds stays out of the product with P = 0
      }
    const int kq = (int)(kb - k0) + 4 * qd;  // key kb + 16t + 4qd + r, counted from k0, is kq + 16t + r
    h8 pf[NQ];  // B operand of O^T: P[query 16i + c][key kb + 16 (j >> 2) + 4qd + (j & 3)] in fp16
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const _Float16* qi = qrow + 16 * i * QLD;
      qqq_f4 st[2];  // S^T: lane l, register r of half t = score of query 16i + c against key kb + 16t + 4qd + r
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        st[t] = qqq_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < SG; ++g) {
          const h8 q0 = *reinterpret_cast<const h8*>(qi + 64 * g), q1 = *reinterpret_cast<const h8*>(qi + 64 * g + 8);
          st[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qqq_kv8_codes_to_h8(kr[t][g][0], kr[t][g][1]), q0, st[t], 0, 0, 0);
          st[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qqq_kv8_codes_to_h8(kr[t][g][2], kr[t][g][3]), q1, st[t], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float sv = (kq + 16 * t + r <= rl[i]) ? st[t][r] * (ksc[t][r] * scale_log2) : -INFINITY;
          st[t][r] = sv;
          mx = fmaxf(mx, sv);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m[i], mx);
      const bool none = mn == -INFINITY;  // the row has seen no key yet, this block included: -inf - (-inf) below
      const float alpha = none ? 1.f : exp2f(m[i] - mn);
      const float mz = none ? 0.f : mn;
      m[i] = mn;
      float ps = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const _Float16 ph = (_Float16)exp2f(st[t][r] - mz);
          pf[i][4 * t + r] = ph;
          ps += (float)ph;
        }
      l[i] = l[i] * alpha + ps;
#pragma unroll
      for (int n = 0; n < NT16; ++n) acc[i][n] *= alpha;
    }
    int qdv = qd;
    asm volatile("" : "+v"(qdv));  // see sel below
#pragma unroll
    for (int g = 0; g < SG; ++g)
#pragma unroll
      for (int tl = 0; tl < 4; ++tl) {
        // byte selection matrix of qqq_paged_kv8_decode_split_kernel, made here from a lane-group index the compiler cannot see through
        const v4i sel = (qdv == tl) ? onehot : v4i{0, 0, 0, 0};
        // V^T rows d = 64g + 16tl + c of keys kb + 16t + 4qd + r (t = 0, 1), in the key order of pf: exact int32 codes, times the key's
        // scale; once for all the tiles
        const v4i z = v4i{0, 0, 0, 0};
        const v4i t0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(vr[0][g], sel, z, 0, 0, 0);
        const v4i t1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(vr[1][g], sel, z, 0, 0, 0);
        const h8 va = {(_Float16)((float)t0[0] * vsc[0][0]), (_Float16)((float)t0[1] * vsc[0][1]), (_Float16)((float)t0[2] * vsc[0][2]),
                       (_Float16)((float)t0[3] * vsc[0][3]), (_Float16)((float)t1[0] * vsc[1][0]), (_Float16)((float)t1[1] * vsc[1][1]),
                       (_Float16)((float)t1[2] * vsc[1][2]), (_Float16)((float)t1[3] * vsc[1][3])};
#pragma unroll
        for (int i = 0; i < NQ; ++i) acc[i][4 * g + tl] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pf[i], acc[i][4 * g + tl], 0, 0, 0);
        if (tl & 1) __builtin_amdgcn_sched_barrier(0);  // two tiles of V^T in flight, as in the decode kernel
      }
  }
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    l[i] += __shfl_xor(l[i], 16);
    l[i] += __shfl_xor(l[i], 32);
  }
  // the lane indices are taken afresh, so that the addresses of the merge are worked out there and not carried through the loop
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  qqq_verify_merge<D, NQ>(lds_o, lds_m, lds_l, acc, m, l, w, tid, bi, kh, sp, h, G, T, p0 - k0, splits, ws_o, ws_ml);
}

// One workgroup per token of the chunk: qqq_decode_combine_kernel's row at the token's own position.
template <int VPT, int NT>
__global__ __launch_bounds__(NT) void qqq_verify_combine_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                                                const long long* __restrict__ start, const long long limit, const int T,
                                                                _Float16* __restrict__ o16, int8_t* __restrict__ xq, float* __restrict__ s1,
                                                                const int h, const int d, const int chunk, const int splits) {
  __shared__ float red_max[NT / 64];
  const int row = blockIdx.x;  // r * T + t
  const int r = row / T;
  const long long p0 = start[r], p = p0 + (row - r * T);
  if (p0 < 0 || p >= limit) return;  // out-of-range token: no fp16 row, no xq, no s1
  qqq_decode_combine_row<VPT, NT>(ws_o, ws_ml, row, p, o16, xq, s1, h, d, chunk, splits, red_max);
}

#endif  // QQQ_AMD_QQQ_VERIFY_HIP_H_
