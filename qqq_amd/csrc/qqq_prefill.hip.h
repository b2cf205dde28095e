// qqq_prefill.hip.h -- paged, ragged, causal prefill attention (include/qqq_amd_prefill.h): one launch for every chunk of a packed batch,
// reading K and V through the block table in place, and a second small launch that quantises the fp16 rows for o_proj.  Part of the single
// translation unit qqq_w4a8.hip.
//
//   qqq_prefill_attn_kernel<D, KV8>   One workgroup (4 waves) per (query tile, KV head).  A query tile is PF_ROWS = 128 rows: TQ = 128 / G
//                                     consecutive tokens of ONE sequence times the G = h / kvh query heads of the KV head (row = token * G +
//                                     g), 32 rows (two 16-column MFMA operands) per wave, so K and V are read once per KV head and tile.
//                                     Keys are walked from key 0 in tiles of PF_KT = 64 keys aligned to the absolute key index, each tile in
//                                     two 32-key steps of qqq_decode_split_kernel's arithmetic (S^T = K Q^T with fp32 accumulation, online
//                                     softmax in the log2 domain, P rounded to fp16, O^T += V^T P^T in fp32).  No split over keys, no atomics:
//                                     a row's result depends on its own query, position and keys only -- a step beyond a row's position is
//                                     an exact no-op for it (alpha = 1, P = 0) -- whatever tile or batch it is computed in.
//     K / V tile    staged once per workgroup in LDS through registers: the global loads of tile i + 1 are issued before the MFMAs of tile i
//                   and stored after them.  An int8 pool is dequantised on the way (K: the exact fp16 codes, the key's scale applied to the
//                   score; V: fp16(float(code) * scale)), so the MFMA loop is one.  K is read back by rows (ds_read_b128, row stride 2D + 16
//                   bytes), V through the gfx950 transposed read ds_read_b64_tr_b16 (row stride 2D + 32 bytes): four keys x sixteen columns
//                   per 16-lane group arrive column-major, which is the A operand of O^T in the key order of P.  Both strides are free of bank
//                   conflicts for their read.
//     block ids     a 16-key group of a tile lies in one block (block_size >= 16); every wave loads whole 16-key groups, so a block id is one
//                   wave-uniform (scalar) table load, fetched a tile ahead of the loads that use it, clamped into [0, num_blocks).
//     safety        a key is clamped to the tile's last key (the position of its last token) before anything is loaded and its score is
//                   masked: slots beyond a sequence's end are never read, table entries beyond (start + count - 1) / block_size neither.
//     (sequence, tile)   found on the device: sequence i owns the tile slots [cu_tokens[i] / TQ + i, ... + ceil(count_i / TQ)) -- disjoint and
//                   increasing in i, so a binary search over cu_tokens finds the owner of a slot -- of m / TQ + b slots in all: the grid
//                   depends on (m, b, h, kvh) only, a surplus workgroup exits.  Slots are handed out from the last one down, the longest
//                   (latest) tiles of a sequence first.
//   qqq_prefill_quant_kernel<VPT, NT> one workgroup per token row: qqq_dynamic_quant_kernel's arithmetic (qqq_act_quant_row) on the fp16 row
//                                     the attention kernel wrote; rows of padding tokens and of out-of-range sequences are skipped.
#ifndef QQQ_AMD_QQQ_PREFILL_HIP_H_
#define QQQ_AMD_QQQ_PREFILL_HIP_H_

static constexpr int PF_WAVES = 4;
static constexpr int PF_NT = PF_WAVES * 64;
static constexpr int PF_ROWS = PF_WAVES * 32;  // query rows (token, query head) of a tile: two 16-row MFMA operands per wave
static constexpr int PF_KT = 64;               // keys of a staged tile: two 32-key softmax steps
static constexpr int PF_QUANT_NT = 512;

typedef short qqq_s4 __attribute__((ext_vector_type(4)));

// the sequence that owns token t (quant kernel) or tile slot `slot` (attention kernel; tq > 0): the largest i in [0, b) with key(i) <= x,
// key(i) = cu[i] (tq == 0) or cu[i] / tq + i.  cu values are clamped into [0, m].  Returns -1 if there is none.
__device__ __forceinline__ int qqq_prefill_find_seq(const int* __restrict__ cu, const int b, const int m, const int tq, const long long x) {
  int lo = 0, hi = b - 1, found = -1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    int c = cu[mid];
    c = c < 0 ? 0 : (c > m ? m : c);
    const long long key = tq ? (long long)(c / tq) + mid : (long long)c;
    if (key <= x) {
      found = mid;
      lo = mid + 1;
    } else {
      hi = mid - 1;
    }
  }
  return found;
}

// ds_read_b64_tr_b16: per 16-lane group a block of 4 rows x 16 columns of 16-bit elements, delivered column-major (lane i of the group gets
// column i, row q in element q); lane 4q + p supplies the address of row q, columns 4p ... 4p + 3.  Every lane must be active.
__device__ __forceinline__ qqq_s4 qqq_prefill_tr_read(const _Float16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) qqq_s4*)(p));
}

template <int D, bool KV8>
__global__ __launch_bounds__(PF_NT) __attribute__((amdgpu_waves_per_eu(2))) void qqq_prefill_attn_kernel(
    const _Float16* __restrict__ q, const void* __restrict__ k_pool_v, const void* __restrict__ v_pool_v, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, const int* __restrict__ block_table, const int table_stride, const int* __restrict__ cu_tokens,
    const long long* __restrict__ start_pos, const long long limit, const float scale_log2, _Float16* __restrict__ o16, const int m,
    const int b, const int h, const int kvh, const int num_blocks, const int lbs, const int nslots) {
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
  const int last = start + tok0 + ntok - 1;  // the tile's last key: nothing beyond it is loaded

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, qd = lane >> 4;
  const int* table = block_table + (size_t)si * table_stride;
  const int bmask = (1 << lbs) - 1;

  // this lane's two query rows (column c of the wave's operands u = 0, 1); a row beyond the tile's tokens repeats the last one, unwritten
  int pos[2];
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
    orow[u] = ((size_t)(cu0 + tok0 + tk) * h + (size_t)kh * G + g) * D;
    const _Float16* qr = q + orow[u] + 8 * qd;
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[u][s] = *reinterpret_cast<const h8*>(qr + 32 * s);
  }
  // the wave's first and last positions (rows are in token order): steps beyond the last are skipped, steps up to the first need no mask
  int t_lo = (32 * w) / G, t_hi = (32 * w + 31) / G;
  t_lo = t_lo < ntok ? t_lo : ntok - 1;
  t_hi = t_hi < ntok ? t_hi : ntok - 1;
  const int wpos_lo = start + tok0 + t_lo, wpos_hi = start + tok0 + t_hi;

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
      int blk = table[__builtin_amdgcn_readfirstlane((int)(gk >> lbs))];
      bid[i] = blk < 0 ? 0 : (blk >= num_blocks ? num_blocks - 1 : blk);
    }
  };
  auto load_tile = [&](const long long kb) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const long long kk = kb + srow0 + RPP * i;
      const int key = (int)(kk < last ? kk : last);  // a key beyond the tile's last is never loaded; its score is masked
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

  fetch_ids(0);
  load_tile(0);
  fetch_ids(PF_KT);
  for (long long kb = 0; kb <= last; kb += PF_KT) {  // 64-bit: last may be close to 2^31
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
      if (k0 > wpos_hi) break;  // wholly above the diagonal for every row of this wave (wave-uniform)
      const bool diag = k0 + 31 > wpos_lo;
      int rel[2];  // the last key of the step each row attends, relative to k0 (diagonal steps only)
#pragma unroll
      for (int u = 0; u < 2; ++u) rel[u] = (int)(pos[u] - k0 < 32 ? pos[u] - k0 : 32);
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
            st[u][t][r] = sv;
            mx = fmaxf(mx, sv);
          }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(mrun[u], mx);  // finite: key 0 is attended by every row, in the first step
        const float alpha = exp2f(mrun[u] - mn);
        mrun[u] = mn;
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const _Float16 ph = (_Float16)exp2f(st[u][t][r] - mn);
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

// One workgroup per token row: quantise the fp16 row the attention kernel wrote.  A padding token (>= cu_tokens[b]) and a token of a
// sequence that does not fit [0, limit) have no row: xq and s1 stay untouched.
template <int VPT, int NT>
__global__ __launch_bounds__(NT) void qqq_prefill_quant_kernel(const _Float16* __restrict__ o16, const int* __restrict__ cu_tokens,
                                                               const long long* __restrict__ start_pos, const long long limit,
                                                               int8_t* __restrict__ xq, float* __restrict__ s1, const int m, const int b,
                                                               const int hd) {
  __shared__ float red_max[NT / 64];
  const int t = blockIdx.x;
  const int si = qqq_prefill_find_seq(cu_tokens, b, m, 0, t);
  if (si < 0) return;
  int cu0 = cu_tokens[si], cu1 = cu_tokens[si + 1];
  cu0 = cu0 < 0 ? 0 : (cu0 > m ? m : cu0);
  cu1 = cu1 < 0 ? 0 : (cu1 > m ? m : cu1);
  if (t >= cu1) return;  // padding (si is the last sequence with tokens at or before t)
  const long long sp = start_pos[si];
  if (sp < 0 || sp + (cu1 - cu0) > limit) return;
  const int tid = threadIdx.x;
  const int nvec = hd >> 3;
  const h8* src = reinterpret_cast<const h8*>(o16 + (size_t)t * hd);
  h8 v[VPT];
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = tid + i * NT;
    if (idx < nvec) v[i] = src[idx];
  }
  qqq_act_quant_row<VPT, NT>(v, nvec, xq + (size_t)t * hd, s1 + t, red_max);
}

#endif  // QQQ_AMD_QQQ_PREFILL_HIP_H_
