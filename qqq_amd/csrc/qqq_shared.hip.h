// qqq_shared.hip.h -- split-K decode attention for rows that share a prefix of their block tables (include/qqq_amd_shared.h): the siblings
// of a family, forked from one prompt, read the prompt's keys once per pack of rows instead of once per row.  Part of the single
// translation unit qqq_w4a8.hip.
//
// The grid, the chunking (decode_split_plan), the workspace layout and the combine launch are qqq_decode_attn_paged's.  What changes is
// which workgroup computes which partial:
//
//   pack            a family's rows fall into packs of `pack` consecutive rows counted from its first row.  The root of row j is family[j]
//                   where that names a row f <= j with family[f] == f, and j itself otherwise; the pack window of row j starts at
//                   root + (j - root) / pack * pack.  Every workgroup of a window sees the same window and the same roots.
//   joint chunk     member j of a window takes split sp jointly iff its pos is in range and (sp + 1) * chunk <= min(shared[j], pos[j] + 1):
//                   the chunk lies wholly inside what it shares, so every key of the chunk is visible to it.  Each wave finds the joint
//                   members of its window with one ballot (lane = slot of the window).  The first of them computes the split for all of
//                   them -- query row slot * G + g of the 16-row tiles, as qqq_verify_split_kernel places tokens -- through its own table
//                   row, and writes every member's partial to that member's workspace slots; the others leave at once.
//   private chunk   a row that does not take the split jointly computes it alone: one slot, the row's own limit.
//
// Both are one code path: a set `live` of slots from row `base` on, a last key, and per query row either that last key or "none".  It is
// qqq_verify_split_kernel's loop with the row limits made per slot, so the blocks a row takes part in, the masks inside them and the order
// of every sum are the decode kernels' for that row alone, and an MFMA column does not see its neighbours: the partials, and with them
// o_fp16, xq and s1, are bit for bit qqq_decode_attn_paged(_kv8)'s.  A tile beyond the last live slot is skipped (workgroup-uniform), so a
// private chunk does the MFMAs of one tile whatever NQ is.
//
// Descriptors are read for rows [0, b) only and decide who computes, never an address: a senseless family or shared value makes rows
// compute alone.  No instantiation uses scratch.
#ifndef QQQ_AMD_QQQ_SHARED_HIP_H_
#define QQQ_AMD_QQQ_SHARED_HIP_H_

static constexpr int SHR_ROWS_MAX = VER_ROWS_MAX;  // query rows (G * pack) of a KV head: four tiles

// waves per SIMD of an instantiation: qqq_verify_waves, but three at NQ = 1 and D = 128 over an fp16 pool too -- the live-slot set beside
// the verify kernel's 124 registers would put four in scratch
constexpr int qqq_shared_waves(const int D, const int NQ, const bool kv8) {
  return (NQ == 1 && D == 128) ? 3 : qqq_verify_waves(D, NQ, kv8);
}

__device__ __forceinline__ int qqq_shared_root(const int* __restrict__ family, const int j) {
  const int f = family[j];
  return (f >= 0 && f <= j && family[f] == f) ? f : j;
}

// What workgroup (sp, bi) computes: slots `live` (bit s = row base + s) up to key p.  False: nothing (out of range, beyond the row's last
// key, or another member of the window computes this row's partial).
__device__ __forceinline__ bool qqq_shared_job(const int* __restrict__ family, const long long* __restrict__ shared,
                                               const long long* __restrict__ pos, const long long limit, const int b, const int pack,
                                               const int sp, const int bi, const int chunk, int& base, unsigned long long& live,
                                               long long& p) {
  const int lane = threadIdx.x & 63;
  const int root = qqq_shared_root(family, bi);
  const int first = root + (bi - root) / pack * pack;
  const long long kend = ((long long)sp + 1) * chunk;
  const int j = first + lane;
  bool joint = false;
  if (lane < pack && j < b && qqq_shared_root(family, j) == root) {
    const long long pj = pos[j];
    if (pj >= 0 && pj < limit) {
      const long long sh = shared[j];
      joint = kend <= (sh < pj + 1 ? sh : pj + 1);
    }
  }
  const unsigned long long mask = __ballot(joint);
  const int me = bi - first;
  if ((mask >> me) & 1) {
    if ((mask & ((1ull << me) - 1)) != 0) return false;  // an earlier member takes the chunk for this row too
    base = first;
    live = mask;
    p = kend - 1;
    return true;
  }
  const long long pb = pos[bi];
  if (pb < 0 || pb >= limit || (long long)sp * chunk > pb) return false;
  base = bi;
  live = 1ull;
  p = pb;
  return true;
}

// Q^T of the live slots into LDS: query row R = slot * G + g of ROWS (zeros elsewhere), rows QLD elements apart
template <int D, int ROWS, int QLD>
__device__ __forceinline__ void qqq_shared_stage_q(_Float16* lds_q, const _Float16* __restrict__ q, const int base,
                                                   const unsigned long long live, const int kh, const int h, const int G) {
  for (int i = threadIdx.x; i < ROWS * (D / 8); i += DEC_WAVES * 64) {
    const int row = i / (D / 8), e = (i - row * (D / 8)) * 8;
    const int slot = row / G, g = row - slot * G;  // slot < 64: ROWS <= 64
    h8 x = h8{};
    if ((live >> slot) & 1) x = *reinterpret_cast<const h8*>(q + (((size_t)base + slot) * h + (size_t)kh * G + g) * D + e);
    *reinterpret_cast<h8*>(lds_q + row * QLD + e) = x;
  }
}

// qqq_verify_merge with slots for tokens: the partials of slot s go to batch row base + s, for the live slots only
template <int D, int NQ>
__device__ __forceinline__ void qqq_shared_merge(float (&lds_o)[DEC_WAVES][16][D], float (&lds_m)[DEC_WAVES][16 * NQ],
                                                 float (&lds_l)[DEC_WAVES][16 * NQ], const qqq_f4 (&acc)[NQ][D / 16], const float (&m)[NQ],
                                                 const float (&l)[NQ], const int w, const int tid, const int base,
                                                 const unsigned long long live, const int nrows, const int kh, const int sp, const int h,
                                                 const int G, const int splits, float* __restrict__ ws_o, float* __restrict__ ws_ml) {
  constexpr int NT16 = D / 16;
  const int ce = tid & 15, qe = (tid >> 4) & 3;
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
        const float f = exp2f(m[i] - M);  // a wave without a block has m = -inf and f = 0; M = -inf only in rows not stored
#pragma unroll
        for (int n = 0; n < NT16; ++n) *reinterpret_cast<qqq_f4*>(&lds_o[w][ce][16 * n + 4 * qe]) = acc[i][n] * f;
      }
      __syncthreads();
      for (int j = tid; j < 16 * (D / 4); j += DEC_WAVES * 64) {
        const int rr = j / (D / 4), e = (j - rr * (D / 4)) * 4;
        const int row = 16 * i + rr;
        const int slot = row / G, g = row - slot * G;
        if (row >= nrows || !((live >> slot) & 1)) continue;  // padding, or a slot that is not part of this job
        qqq_f4 o = *reinterpret_cast<const qqq_f4*>(&lds_o[0][rr][e]);
#pragma unroll
        for (int ww = 1; ww < DEC_WAVES; ++ww) o += *reinterpret_cast<const qqq_f4*>(&lds_o[ww][rr][e]);
        const size_t part = (((size_t)base + slot) * h + (size_t)kh * G + g) * splits + sp;
        *reinterpret_cast<qqq_f4*>(ws_o + part * D + e) = o;
      }
      __syncthreads();
    }
  }
  if (tid < nrows) {
    const int slot = tid / G, g = tid - slot * G;
    if ((live >> slot) & 1) {
      float M = lds_m[0][tid];
#pragma unroll
      for (int ww = 1; ww < DEC_WAVES; ++ww) M = fmaxf(M, lds_m[ww][tid]);
      float L = 0.f;
#pragma unroll
      for (int ww = 0; ww < DEC_WAVES; ++ww) L += lds_l[ww][tid] * exp2f(lds_m[ww][tid] - M);
      const size_t part = (((size_t)base + slot) * h + (size_t)kh * G + g) * splits + sp;
      reinterpret_cast<float2*>(ws_ml)[part] = make_float2(M, L);
    }
  }
}

template <int D, int NQ>
__global__ __launch_bounds__(DEC_WAVES * 64) __attribute__((amdgpu_waves_per_eu(qqq_shared_waves(D, NQ, false)))) void qqq_shared_split_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ k_pool, const _Float16* __restrict__ v_pool,
    const int* __restrict__ block_table, const int table_stride, const long long* __restrict__ pos, const long long limit,
    const int* __restrict__ family, const long long* __restrict__ shared, const int pack, const float scale_log2,
    float* __restrict__ ws_o, float* __restrict__ ws_ml, const int h, const int kvh, const int num_blocks, const int lbs, const int chunk,
    const int splits) {
  constexpr int KS = D / 32;    // k-steps of S^T = K Q^T
  constexpr int NT16 = D / 16;  // 16-column tiles of O^T
  constexpr int ROWS = 16 * NQ, QLD = D + 8;
  __shared__ float lds_o[DEC_WAVES][16][D];
  __shared__ float lds_m[DEC_WAVES][ROWS], lds_l[DEC_WAVES][ROWS];
  static_assert(ROWS * QLD * sizeof(_Float16) <= sizeof(lds_o), "Q^T waits in the merge buffer");
  const int sp = blockIdx.x, kh = blockIdx.y, bi = blockIdx.z;
  int base;
  unsigned long long live;
  long long p;  // the last key any slot of the job may see
  if (!qqq_shared_job(family, shared, pos, limit, (int)gridDim.z, pack, sp, bi, chunk, base, live, p)) return;
  const long long k0 = (long long)sp * chunk;
  const long long last = (k0 + chunk - 1 < p) ? k0 + chunk - 1 : p;
  const int G = h / kvh;
  const int nrows = G * (64 - __builtin_clzll(live));  // query rows up to the last live slot; <= ROWS by the host's choice of NQ
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform and known to be: the table loads are scalar
  const int c = lane & 15, qd = lane >> 4;
  const int* table = block_table + (size_t)bi * table_stride;  // a joint chunk is read through the computing member's own row
  const int bmask = (1 << lbs) - 1;

  _Float16* lds_q = reinterpret_cast<_Float16*>(&lds_o[0][0][0]);
  qqq_shared_stage_q<D, ROWS, QLD>(lds_q, q, base, live, kh, h, G);
  __syncthreads();
  const _Float16* qrow = lds_q + c * QLD + 8 * qd;  // B operand of S^T: query row 16i + c, head elements 32s + 8qd + j

  // the last key of query row 16i + c, counted from k0: below 0 for padding rows and slots that are not part of the job
  int rl[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int slot = (16 * i + c) / G;
    rl[i] = ((live >> slot) & 1) ? (int)(last - k0) : -1;
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
      key = key > p ? p : key;  // rows past the job's last key load a valid row; their scores are masked below
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
      if (16 * i >= nrows) continue;  // workgroup-uniform: no live slot in this tile or behind it
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
      const bool none = mn == -INFINITY;  // a row that is not part of the job sees no key: -inf - (-inf) below
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
        for (int i = 0; i < NQ; ++i)
          if (16 * i < nrows) acc[i][2 * s + hh] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pf[i], acc[i][2 * s + hh], 0, 0, 0);
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
  qqq_shared_merge<D, NQ>(lds_o, lds_m, lds_l, acc, m, l, w, tid, base, live, nrows, kh, sp, h, G, splits, ws_o, ws_ml);
}

template <int D, int NQ>
__global__ __launch_bounds__(DEC_WAVES * 64) __attribute__((amdgpu_waves_per_eu(qqq_shared_waves(D, NQ, true)))) void qqq_shared_kv8_split_kernel(
    const _Float16* __restrict__ q, const int8_t* __restrict__ k_pool, const int8_t* __restrict__ v_pool, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, const int* __restrict__ block_table, const int table_stride, const long long* __restrict__ pos,
    const long long limit, const int* __restrict__ family, const long long* __restrict__ shared, const int pack, const float scale_log2,
    float* __restrict__ ws_o, float* __restrict__ ws_ml, const int h, const int kvh, const int num_blocks, const int lbs, const int chunk,
    const int splits) {
  constexpr int SG = D / 64;    // 64-element segments of a head row: one 16-byte load per lane each
  constexpr int NT16 = D / 16;  // 16-column tiles of O^T
  constexpr int ROWS = 16 * NQ, QLD = D + 8;
  __shared__ float lds_o[DEC_WAVES][16][D];
  __shared__ float lds_m[DEC_WAVES][ROWS], lds_l[DEC_WAVES][ROWS];
  static_assert(ROWS * QLD * sizeof(_Float16) <= sizeof(lds_o), "Q^T waits in the merge buffer");
  const int sp = blockIdx.x, kh = blockIdx.y, bi = blockIdx.z;
  int base;
  unsigned long long live;
  long long p;  // the last key any slot of the job may see
  if (!qqq_shared_job(family, shared, pos, limit, (int)gridDim.z, pack, sp, bi, chunk, base, live, p)) return;
  const long long k0 = (long long)sp * chunk;
  const long long last = (k0 + chunk - 1 < p) ? k0 + chunk - 1 : p;
  const int G = h / kvh;
  const int nrows = G * (64 - __builtin_clzll(live));  // query rows up to the last live slot; <= ROWS by the host's choice of NQ
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform and known to be: a block's addresses stay in SGPRs
  const int c = lane & 15, qd = lane >> 4;
  const int* table = block_table + (size_t)bi * table_stride;  // a joint chunk is read through the computing member's own row
  const int bmask = (1 << lbs) - 1;

  _Float16* lds_q = reinterpret_cast<_Float16*>(&lds_o[0][0][0]);
  qqq_shared_stage_q<D, ROWS, QLD>(lds_q, q, base, live, kh, h, G);
  __syncthreads();
  const _Float16* qrow = lds_q + c * QLD + 16 * qd;  // elements 64g + 16qd + 8u + j: the order of a K load's bytes
  v4i onehot;  // byte c of the lane's 16
#pragma unroll
  for (int i = 0; i < 4; ++i) onehot[i] = ((c >> 2) == i) ? (1 << (8 * (c & 3))) : 0;

  // the last key of query row 16i + c, counted from k0: below 0 for padding rows and slots that are not part of the job
  int rl[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int slot = (16 * i + c) / G;
    rl[i] = ((live >> slot) & 1) ? (int)(last - k0) : -1;
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
    const int rem = (int)(last - kb < DEC_BLOCK - 1 ? last - kb : DEC_BLOCK - 1);  // the block's last key any slot attends
    const int pin = (int)(p - kb < DEC_BLOCK - 1 ? p - kb : DEC_BLOCK - 1);        // the job's last key, if it lies in the block
    v4i kr[2][SG], vr[2][SG];
    qqq_f4 ksc[2], vsc[2];  // scales of keys kb + 16t + 4qd + r
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      // a half's addresses are a scalar base (its block's row of this KV head) plus 32-bit lane offsets inside the block
      const int8_t* kblk = k_pool + brow[t] * D;
      const int8_t* vblk = v_pool + brow[t] * D;
      const float* ksb = k_scale + brow[t];
      const float* vsb = v_scale + brow[t];
      const int key = 16 * t + c < pin ? 16 * t + c : pin;  // rows past the job's last key load that key; their scores are masked below
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
      if (16 * i >= nrows) continue;  // workgroup-uniform: no live slot in this tile or behind it
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
      const bool none = mn == -INFINITY;  // a row that is not part of the job sees no key: -inf - (-inf) below
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
        for (int i = 0; i < NQ; ++i)
          if (16 * i < nrows) acc[i][4 * g + tl] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pf[i], acc[i][4 * g + tl], 0, 0, 0);
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
  qqq_shared_merge<D, NQ>(lds_o, lds_m, lds_l, acc, m, l, w, tid, base, live, nrows, kh, sp, h, G, splits, ws_o, ws_ml);
}

#endif  // QQQ_AMD_QQQ_SHARED_HIP_H_
