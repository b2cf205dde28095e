// qqq_moe.hip.h -- mixture-of-experts layers: the router (softmax, top-k, stable counting sort by expert), the grouped W4A8 GEMM over
// routed rows, and the weighted combine (include/qqq_amd_moe.h states the arithmetic).
// Part of the single translation unit qqq_w4a8.hip (see its header comment for the design).
#ifndef QQQ_AMD_QQQ_MOE_HIP_H_
#define QQQ_AMD_QQQ_MOE_HIP_H_

#define MOE_MAX_E 256
#define MOE_MAX_TOPK 16
#define MOE_ROUTE_WAVES 4   // token rows (one wave each) per workgroup of the selection kernel
#define MOE_SORT_WAVES 16   // the sort is ONE workgroup of 1024 threads that walks the pairs in chunks of 1024
#define MOE_GEMM_WAVES 4    // waves of a grouped-GEMM workgroup: they split K (four: a 512-register budget per lane, the 64-row body keeps its 128 accumulators and its ring without scratch)
#define MOE_PASS_ROWS 64    // rows of one pass over an expert's weights: up to four 16-token MFMA tiles

// ------------------------------------------------------------------------------------------
// routing, launch 1: softmax + top-k, one wave per token row
// ------------------------------------------------------------------------------------------
// Lane l holds the logits of experts l, l + 64, l + 128, l + 192.  The selection is a max over (probability, lower index) among the
// entries not yet taken; `taken` is a flag of its own and a NaN probability orders below every number, so whatever the row holds
// the top_k ids are distinct and inside [0, E).
__device__ __forceinline__ float moe_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float moe_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(MOE_ROUTE_WAVES * 64) void qqq_moe_topk_kernel(const _Float16* __restrict__ logits, const int ld,
                                                                             int* __restrict__ ids, float* __restrict__ w, const int T,
                                                                             const int E, const int top_k, const int renorm) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * MOE_ROUTE_WAVES + (threadIdx.x >> 6);
  if (t >= T) return;  // (whole waves leave: no barrier below)
  const _Float16* row = logits + (size_t)t * ld;
  float x[4], p[4];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = lane + 64 * i;
    x[i] = e < E ? (float)row[e] : -INFINITY;
    mx = fmaxf(mx, x[i]);  // (fmaxf drops a NaN operand: a row with NaNs keeps a finite maximum where it has one)
  }
  mx = moe_wave_max(mx);
  float part = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[i] = lane + 64 * i < E ? expf(x[i] - mx) : 0.0f;
    part += p[i];
  }
  const float sum = moe_wave_sum(part);
  // selection keys: u = exp(x - max) orders the experts as their probabilities u / sum do (one positive divisor), so the keys are u's
  // bits as an ordered unsigned (u >= 0; NaN -> 0) above nine bits that hold 511 - e: among equal u the lower expert wins and every key
  // is > 0; an entry past E or already taken is not `live`
  unsigned long long key[4];
  bool live[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = lane + 64 * i;
    live[i] = e < E;
    const unsigned bits = p[i] == p[i] ? __float_as_uint(p[i]) : 0u;
    key[i] = ((unsigned long long)bits << 9) | (unsigned long long)(511 - e);
  }
  float sel_p = 0.0f, sel_sum = 0.0f;  // lane j keeps slot j's u
  int sel_e = 0;
  for (int j = 0; j < top_k; ++j) {
    unsigned long long best = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (live[i] && key[i] > best) best = key[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(best, o);
      best = other > best ? other : best;
    }
    const int e = 511 - (int)(best & 511);  // top_k <= E live entries at the start, one taken per round: best > 0
    const int owner = e & 63, slot = e >> 6;
    float pe = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i == slot) {
        pe = p[i];
        if (lane == owner) live[i] = false;
      }
    pe = __shfl(pe, owner);
    sel_sum += pe;  // slot order j = 0, 1, ...: every lane holds the same bits
    if (lane == j) {
      sel_p = pe;
      sel_e = e;
    }
  }
  if (lane < top_k) {
    ids[(size_t)t * top_k + lane] = sel_e;
    w[(size_t)t * top_k + lane] = sel_p / (renorm ? sel_sum : sum);  // (renormalised: the row's sum cancels, one division in all)
  }
}

// ------------------------------------------------------------------------------------------
// routing, launch 2: stable counting sort of the pairs by expert, ONE workgroup
// ------------------------------------------------------------------------------------------
// A pure function of ids[]: the histogram uses LDS atomics (a count does not depend on the order of its increments), every POSITION
// comes from ballots and scans.  Pairs are walked in chunks of 1024 in ascending p; inside a chunk a lane's rank among the lanes of its
// wave with the same expert is a popcount over a ballot mask, the waves' counts are scanned per expert in wave order, and the running
// base of every expert carries over to the next chunk.  An id outside [0, E) (the selection kernel writes none) counts as E - 1.
__global__ __launch_bounds__(MOE_SORT_WAVES * 64) void qqq_moe_sort_kernel(const int* __restrict__ ids, int* __restrict__ offsets,
                                                                            int* __restrict__ order, const int P, const int E) {
  __shared__ int base[MOE_MAX_E];
  __shared__ int wcnt[MOE_SORT_WAVES][MOE_MAX_E];
  __shared__ int wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NT = MOE_SORT_WAVES * 64;

  if (tid < MOE_MAX_E) base[tid] = 0;
  __syncthreads();
  for (int p = tid; p < P; p += NT) {
    const int e = ids[p];
    atomicAdd(&base[(unsigned)e < (unsigned)E ? e : E - 1], 1);
  }
  __syncthreads();
  // exclusive scan of the E <= 256 counts by the first four waves
  int cnt = 0, incl = 0;
  if (tid < MOE_MAX_E) {
    cnt = tid < E ? base[tid] : 0;
    incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (lane == 63) wtot[wave] = incl;
  }
  __syncthreads();
  if (tid < MOE_MAX_E) {
    int before = 0;
    for (int v = 0; v < wave; ++v) before += wtot[v];
    const int excl = before + incl - cnt;
    base[tid] = excl;
    if (tid < E) offsets[tid] = excl;
    if (tid == E - 1) offsets[E] = excl + cnt;
  }
  __syncthreads();

  for (int p0 = 0; p0 < P; p0 += NT) {
    for (int i = tid; i < MOE_SORT_WAVES * MOE_MAX_E; i += NT) (&wcnt[0][0])[i] = 0;
    __syncthreads();
    const int p = p0 + tid;
    const bool valid = p < P;
    int e = valid ? ids[p] : 0;
    e = (unsigned)e < (unsigned)E ? e : E - 1;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (e >> b) & 1;
      const unsigned long long has = __ballot(bit);
      peers &= bit ? has : ~has;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wcnt[wave][e] = __popcll(peers);
    __syncthreads();
    if (tid < E) {
      int run = base[tid];
      for (int v = 0; v < MOE_SORT_WAVES; ++v) {
        const int c = wcnt[v][tid];
        wcnt[v][tid] = run;
        run += c;
      }
      base[tid] = run;
    }
    __syncthreads();
    if (valid) {
      const int pos = wcnt[wave][e] + rank;
      if ((unsigned)pos < (unsigned)P) order[pos] = p;  // (always true: the positions of a chunk are a permutation of a range)
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------
// the grouped GEMM
// ------------------------------------------------------------------------------------------
// grid = (ceil(N / 128) column strips, E experts); block = MOE_GEMM_WAVES * 64; no split-K across workgroups, no workspace.
// The operand roles, the lane maps and the per-step loads are the stream kernel's (qqq_stream.hip.h): a lane loads the 64 packed bytes
// that hold all 16 k of its 8 weight columns, the unpack doubles as the register transpose, and the activations are the MFMA "B" operand,
// 16 contiguous int8 of one token row.  What is its own: the expert's weight slice comes from blockIdx.y, a lane's activation row comes
// from order[] (the gather is the address), the rows of an expert are walked in passes of up to 64 with the tile count of each pass picked
// from what is left, and the epilogue scatters to pair order.  The waves take the 64-k steps round-robin and fold their int32 partial tiles
// in LDS (integer adds: the sum has one value whatever the arrival order), the readers leave the tile zero for the next pass.
struct qqq_moe_gemm_args {
  const int8_t* xq;
  const float* s1;
  const unsigned char* B;
  const float* s2;
  const _Float16* s3;
  const int* offsets;
  const int* order;
  _Float16* D;
  int P, R, N, K, a_div;
};

template <int MT, bool GROUPED, int PF>
__device__ __forceinline__ void moe_gemm_pass(const qqq_moe_gemm_args& a, int* __restrict__ red, const unsigned char* __restrict__ bptr,
                                              const _Float16* __restrict__ sptr, const float* __restrict__ s2e, const int off,
                                              const int row0, const int cnt, const int strip) {
  constexpr int WAVES = MOE_GEMM_WAVES;
  constexpr int NQ = MT * 8;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, h = lane >> 4;
  const int N = a.N, K = a.K;
  const size_t rowbytes = (size_t)N * 8;

  // the activation rows of this pass: position off + r of order[] names the pair, the pair names the row; a position past the
  // expert's count re-reads the last one (its output is dropped), and a pair index is held inside [0, P) whatever order[] holds
  const int8_t* xptr[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    int r = row0 + 16 * mt + j;
    if (r >= cnt) r = cnt - 1;
    int p = a.order[off + r];
    p = p < 0 ? 0 : (p >= a.P ? a.P - 1 : p);
    int ar = p / a.a_div;
    if (ar >= a.R) ar = a.R - 1;
    xptr[mt] = a.xq + (size_t)ar * K + 16 * h;
  }

  v4i acc[MT][4][2];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      acc[mt][jt][0] = (v4i){0, 0, 0, 0};
      acc[mt][jt][1] = (v4i){0, 0, 0, 0};
    }

  auto load_step = [&](const int s, StreamStep<MT>& r) {
    const unsigned char* p = bptr + (size_t)(4 * s) * rowbytes;
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) r.w[kq] = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p + 16 * kq));  // an expert's strip is read once per pass
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) r.x[mt] = *reinterpret_cast<const v4i*>(xptr[mt] + 64 * s);
    if constexpr (GROUPED) r.sc = *reinterpret_cast<const h8*>(sptr + (size_t)(s >> 1) * N);
  };
  auto compute_step = [&](const StreamStep<MT>& r) {
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      v4i a0, a1;
      h2 sb0 = {(_Float16)0, (_Float16)0}, sb1 = sb0;
      if constexpr (GROUPED) {
        sb0 = (h2){r.sc[2 * jt], r.sc[2 * jt]};
        sb1 = (h2){r.sc[2 * jt + 1], r.sc[2 * jt + 1]};
      }
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) {
        int w0, w1;
        unpack_pair<GROUPED>(r.w[kq][jt], sb0, sb1, w0, w1);
        a0[kq] = w0;
        a1[kq] = w1;
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        acc[mt][jt][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, r.x[mt], acc[mt][jt][0], 0, 0, 0);
        acc[mt][jt][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, r.x[mt], acc[mt][jt][1], 0, 0, 0);
      }
    }
  };

  // PF steps (4 KiB of weights each) in flight per wave; a wave's steps are wave, wave + WAVES, ...  The steady-state loop is branch-free
  // (counted waits), the ragged tail -- all there is at the K of an expert matrix -- takes the checked path.
  const int ks_end = K >> 6;
  StreamStep<MT> ring[PF];
  int s = wave;
  if (s + (2 * PF - 1) * WAVES < ks_end) {
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      load_step(s + q * WAVES, ring[q]);
      __builtin_amdgcn_sched_barrier(0);
    }
    for (; s + (2 * PF - 1) * WAVES < ks_end; s += PF * WAVES) {
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        compute_step(ring[q]);
        __builtin_amdgcn_sched_barrier(0);
        load_step(s + (q + PF) * WAVES, ring[q]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < PF; ++q)
      if (s + q * WAVES < ks_end) load_step(s + q * WAVES, ring[q]);
  }
  for (; s < ks_end; s += PF * WAVES) {
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      const int sc = s + q * WAVES;
      if (sc < ks_end) {
        compute_step(ring[q]);
        const int sn = sc + PF * WAVES;
        if (sn < ks_end) load_step(sn, ring[q]);
      }
    }
  }

  // fold the waves' partial tiles (red is zero on entry)
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          __hip_atomic_fetch_add(&red[(((mt * 4 + jt) * 2 + b) * 4 + r) * 64 + lane], acc[mt][jt][b][r], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();

  // write out: item = (q = (mt, jt, b), lane) -> 4 consecutive n of one pair's row; the reader zeroes what it read
  for (int it = tid; it < NQ * 64; it += WAVES * 64) {
    const int q = it >> 6, ln = it & 63;
    const int mt = q >> 3, jt = (q >> 1) & 3, b = q & 1, qd = ln >> 4;
    const int r = row0 + 16 * mt + (ln & 15);
    const int n = strip * 128 + 64 * (qd >> 1) + 16 * jt + 8 * b + 4 * (qd & 1);
    int* rp = &red[(q * 4) * 64 + ln];
    const v4i v = {rp[0], rp[64], rp[128], rp[192]};
    rp[0] = 0;
    rp[64] = 0;
    rp[128] = 0;
    rp[192] = 0;
    if (r < cnt && n < N) {
      const int p = a.order[off + r];
      const int ar = p / a.a_div;
      if ((unsigned)p < (unsigned)a.P && ar < a.R) epilogue_store4(v[0], v[1], v[2], v[3], p, n, N, a.s1[ar], s2e, a.D, nullptr);
    }
  }
  __syncthreads();
}

template <bool GROUPED>
__global__ __launch_bounds__(MOE_GEMM_WAVES * 64) void qqq_moe_gemm_kernel(const qqq_moe_gemm_args a) {
  __shared__ int red[32 * 4 * 64];
  const int e = blockIdx.y, strip = blockIdx.x;
  int off = a.offsets[e], end = a.offsets[e + 1];
  off = off < 0 ? 0 : (off > a.P ? a.P : off);
  end = end < off ? off : (end > a.P ? a.P : end);
  const int cnt = end - off;
  if (cnt == 0) return;  // most workgroups of a decode step: their expert was not chosen

  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < 32 * 4 * 64; i += MOE_GEMM_WAVES * 64) red[i] = 0;
  __syncthreads();

  const int j = lane & 15, h = lane >> 4, g = j >> 3, c = j & 7;
  const int N = a.N, K = a.K;
  const int ngroups = N >> 6;
  int ng = strip * 2 + g;
  if (ng >= ngroups) ng = ngroups - 1;  // clamp (N % 128 == 64): loads stay legal, output dropped
  const unsigned char* bptr = a.B + (size_t)e * ((size_t)K * N / 2) + (size_t)h * ((size_t)N * 8) + (size_t)ng * 512 + c * 64;
  const _Float16* sptr = GROUPED ? a.s3 + (size_t)e * (size_t)(K >> 7) * N + (size_t)ng * 64 + c * 8 : nullptr;
  const float* s2e = a.s2 + (size_t)e * N;

  for (int row0 = 0; row0 < cnt; row0 += MOE_PASS_ROWS) {
    const int left = cnt - row0;  // workgroup-uniform: every wave takes the same body, the barriers inside line up
    if (left <= 16) moe_gemm_pass<1, GROUPED, 4>(a, red, bptr, sptr, s2e, off, row0, cnt, strip);
    else if (left <= 32) moe_gemm_pass<2, GROUPED, 3>(a, red, bptr, sptr, s2e, off, row0, cnt, strip);
    else if (left <= 48) moe_gemm_pass<3, GROUPED, 2>(a, red, bptr, sptr, s2e, off, row0, cnt, strip);
    else moe_gemm_pass<4, GROUPED, 2>(a, red, bptr, sptr, s2e, off, row0, cnt, strip);
  }
}

static void moe_gemm_launch(bool grouped, const dim3 grid, hipStream_t stream, const qqq_moe_gemm_args& a) {
  if (grouped) hipLaunchKernelGGL(qqq_moe_gemm_kernel<true>, grid, dim3(MOE_GEMM_WAVES * 64), 0, stream, a);
  else hipLaunchKernelGGL(qqq_moe_gemm_kernel<false>, grid, dim3(MOE_GEMM_WAVES * 64), 0, stream, a);
}

// ------------------------------------------------------------------------------------------
// the combine: out[t, :] = sum over the token's top_k pairs of w * y, one launch
// ------------------------------------------------------------------------------------------
// A thread owns 8 consecutive columns of one token (16-byte loads and one 16-byte store); products and sums are separate f32
// operations, in slot order onto +0.0f, one rounding to fp16 at the end.
__global__ __launch_bounds__(256) void qqq_moe_combine_kernel(const _Float16* __restrict__ y, const float* __restrict__ w,
                                                               _Float16* __restrict__ out, const int H, const int top_k) {
  const int t = blockIdx.x;
  const int h0 = (blockIdx.y * 256 + threadIdx.x) * 8;
  if (h0 >= H) return;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
  for (int jj = 0; jj < top_k; ++jj) {
    const size_t p = (size_t)t * top_k + jj;
    const float wj = w[p];
    const h8 v = *reinterpret_cast<const h8*>(y + p * H + h0);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(wj, (float)v[i]));
  }
  h8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (_Float16)acc[i];
  *reinterpret_cast<h8*>(out + (size_t)t * H + h0) = o;
}

#endif  // QQQ_AMD_QQQ_MOE_HIP_H_
