// qqq_sample.hip.h -- the fused token sampler (include/qqq_amd_sample.h): temperature, top-k, top-p and the draw for every row of a batch of
// fp16 logits in ONE launch, all per-row parameters read from device memory.  Part of the single translation unit qqq_w4a8.hip.
//
//   qqq_sample_tokens_kernel   One workgroup (16 waves) per row; the row is walked three to six times (the first walk from HBM or wherever the
//                              head GEMM left it, the others from the L2), 16 bytes per lane and instruction, the vocab % 8 tail by scalar
//                              loads: the padding columns vocab ... ld - 1 are never read.
//     key           a logit's 16 bits mapped to an unsigned key that orders like the value: -0 joins +0, NaN and -inf become key 0 ("no
//                   weight"); finite values are 0x0400 ... 0xfbff, +inf 0xfc00.  Both cuts are thresholds on the key.
//     walk 0        the maximum key and its lowest index (one 64-bit max over key << 32 | ~index), and whether any logit is finite.  A row
//                   without one returns 0; a greedy row (T <= 0, T NaN, k == 1) returns that index.
//     weights       w = 1 for the maximum's key, else exp2((l - l_max) * (log2 e / T)) in f32, then TRUNCATED TO A MULTIPLE OF 2^-44 and
//                   summed as 64-bit integers (at most 2^18 terms of at most 2^44).  Integer sums are exact and do not depend on their
//                   order: histogram masses from LDS atomics, the total and the running sum in token order all agree to the bit, from run to
//                   run and from launch to graph replay, and the draw always finds its token.
//     radix select  two levels of 256 bins (the key's high byte, then the low byte inside the chosen bin), counts for top-k and masses for
//                   top-p, in LDS with ds_add_u32 / ds_add_u64 into one of 8 copies per bin (lane & 7; the copies of a bin are neighbours
//                   in LDS, so lanes that agree on a bin collide only 8 apart).  The level-1 walk fills counts and masses together; top-k's
//                   level-2 walk does too, and top-p reuses it when its cut falls into the same bin, else walks once more for its own.
//                   "The largest bin whose suffix sum from the top reaches `need`" is the one primitive behind both cuts: need = k on the
//                   counts; need = W - floor((1 - p) W) on the masses of the kept keys (a key stays iff the mass of the keys above it is
//                   below that).  Every wave evaluates it redundantly from LDS with a 64-lane scan: no broadcast step.
//     draw          each wave owns a contiguous sixteenth of the row, read 64 vectors at a time in token order.  Walk A: every wave's total
//                   mass; W2 and target = floor(u W2) follow, and the wave that holds the target.  Walk B: that wave alone goes over its
//                   part again, 512 tokens per step, until the running sum passes the target, then a lane scan and eight elements.
#ifndef QQQ_AMD_QQQ_SAMPLE_HIP_H_
#define QQQ_AMD_QQQ_SAMPLE_HIP_H_

static constexpr int SMP_WAVES = 16;
static constexpr int SMP_NT = SMP_WAVES * 64;
static constexpr int SMP_COPIES = 8;                 // histogram copies per bin
static constexpr float SMP_ONE = 17592186044416.f;   // 2^44: the fixed-point weight of the maximum
static constexpr int SMP_MAX_VOCAB = 262144;

typedef unsigned long long qqq_u64;

__device__ __forceinline__ unsigned qqq_sample_key(const unsigned b) {  // b: the 16 bits of an fp16
  if ((b & 0x7fffu) > 0x7c00u || b == 0xfc00u) return 0u;  // NaN, -inf
  if (b == 0x8000u) return 0x8000u;                         // -0 == +0
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

__device__ __forceinline__ float qqq_sample_value(const unsigned key) {  // the value of a key other than 0
  const unsigned b = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);
  return (float)__builtin_bit_cast(_Float16, (unsigned short)b);
}

// the fixed-point weight of a logit: 0 below the cut `ks` (>= 1, so an invalid key has none)
__device__ __forceinline__ qqq_u64 qqq_sample_weight(const unsigned b, const unsigned key, const unsigned ks, const unsigned kmax,
                                                     const float lmax, const float c) {
  if (key < ks) return 0ull;
  if (key == kmax) return (qqq_u64)SMP_ONE;
  const float a = ((float)__builtin_bit_cast(_Float16, (unsigned short)b) - lmax) * c;  // <= 0, or NaN (inf - inf, 0 * inf)
  return a <= 0.f ? (qqq_u64)(exp2f(a) * SMP_ONE) : 0ull;
}

// vector v (tokens 8v ... 8v + 7) of a row; elements from `vocab` on come back as NaN (key 0) without being read
__device__ __forceinline__ v4u qqq_sample_load(const unsigned short* __restrict__ row, const int v, const int vocab) {
  const int j0 = 8 * v;
  if (j0 + 8 <= vocab) return *reinterpret_cast<const v4u*>(row + j0);
  v4u x = {0x7e007e00u, 0x7e007e00u, 0x7e007e00u, 0x7e007e00u};
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (j0 + e < vocab) {
      const unsigned b = row[j0 + e];
      x[e >> 1] = (e & 1) ? ((x[e >> 1] & 0x0000ffffu) | (b << 16)) : ((x[e >> 1] & 0xffff0000u) | b);
    }
  return x;
}

__device__ __forceinline__ unsigned qqq_sample_bits(const v4u x, const int e) { return (e & 1) ? (x[e >> 1] >> 16) : (x[e >> 1] & 0xffffu); }

__device__ __forceinline__ qqq_u64 qqq_sample_wave_sum(qqq_u64 x) {
#pragma unroll
  for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

__device__ __forceinline__ qqq_u64 qqq_sample_wave_scan(qqq_u64 x, const int lane) {  // inclusive, lanes ascending
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const qqq_u64 y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  return x;
}

// the sum of h[0 ... 255], by every wave for itself
__device__ __forceinline__ qqq_u64 qqq_sample_total(const qqq_u64* h, const int lane) {
  return qqq_sample_wave_sum(h[4 * lane] + h[4 * lane + 1] + h[4 * lane + 2] + h[4 * lane + 3]);
}

// The largest bin B with h[B] + ... + h[255] >= need (need >= 1), and `above` = h[B + 1] + ... + h[255]; bin 0 and all but h[0] if the total
// falls short.  Every wave for itself: lane l owns the bins 255 - 4l ... 252 - 4l, so a scan over the lanes is the suffix sum from the top.
__device__ __forceinline__ int qqq_sample_select(const qqq_u64* h, const qqq_u64 need, qqq_u64& above, const int lane) {
  qqq_u64 a[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = h[255 - 4 * lane - j];
  const qqq_u64 s = a[0] + a[1] + a[2] + a[3];
  const qqq_u64 incl = qqq_sample_wave_scan(s, lane);
  const qqq_u64 hit = __ballot(incl >= need);
  int bin = 0;
  qqq_u64 run = incl - s;
  if (hit == 0ull) {
    run = incl - a[3];  // lane 63: everything above bin 0
    const int src = 63;
    above = __shfl(run, src);
    return 0;
  }
  const int src = __ffsll((long long)hit) - 1;
  bool done = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!done && run + a[j] >= need) {
      bin = 255 - 4 * lane - j;
      done = true;
    }
    if (!done) run += a[j];
  }
  above = __shfl(run, src);
  return __shfl(bin, src);
}

// One walk over the row that fills the histograms' copies: L2 = false by the key's high byte, L2 = true by the low byte of the keys whose
// high byte is `sel`.  Counts take every token (key 0 included), masses the keys with a weight.
template <bool L2>
__device__ __forceinline__ void qqq_sample_hist(const unsigned short* __restrict__ row, const int vocab, const int nvec, const unsigned sel,
                                                const bool counts, const bool masses, const unsigned kmax, const float lmax, const float c,
                                                unsigned* hc, qqq_u64* hm, const int tid) {
  const int cp = tid & (SMP_COPIES - 1);
  for (int v = tid; v < nvec; v += SMP_NT) {
    const v4u x = qqq_sample_load(row, v, vocab);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (8 * v + e >= vocab) continue;
      const unsigned b = qqq_sample_bits(x, e);
      const unsigned key = qqq_sample_key(b);
      if (L2 && (key >> 8) != sel) continue;
      const int slot = (int)(L2 ? (key & 0xffu) : (key >> 8)) * SMP_COPIES + cp;
      if (counts) atomicAdd(&hc[slot], 1u);
      if (masses) {
        const qqq_u64 wf = qqq_sample_weight(b, key, 1u, kmax, lmax, c);
        if (wf) atomicAdd(&hm[slot], wf);
      }
    }
  }
}

// Where a row's variate comes from and what the one lane that ends up holding the row's token does with it: qqq_sample_tokens reads u[r]
// and stores the token; the decode loop's step kernel (qqq_step.hip.h) indexes u by the row's tick and advances the row's state.
struct qqq_sample_store {
  const float* __restrict__ uu;
  long long* __restrict__ tokens;
  __device__ __forceinline__ float variate(const int r) const { return uu[r]; }
  __device__ __forceinline__ void operator()(const int r, const long long tok) const { tokens[r] = tok; }
};

// The sampler of one row by one workgroup, shared by every kernel that draws a token: every lane calls emit.variate(r) in front of the
// first barrier, and `emit(r, token)` is called exactly once, by one lane, behind it.
template <class Emit>
__device__ __forceinline__ void qqq_sample_row(const unsigned short* __restrict__ logits, const int ld, const float* __restrict__ temperature,
                                               const int* __restrict__ top_k, const float* __restrict__ top_p, const int vocab, const int r,
                                               const Emit emit) {
  __shared__ unsigned hc[256 * SMP_COPIES];
  __shared__ qqq_u64 hm[256 * SMP_COPIES];
  __shared__ qqq_u64 cnt[256], m1[256], m2[256];
  __shared__ qqq_u64 red[SMP_WAVES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned short* row = logits + (size_t)r * ld;
  const int nvec = (vocab + 7) >> 3;
  const float T = temperature[r];
  const int k = top_k[r];
  const float p = top_p[r];
  const float u = emit.variate(r);

  // ---- walk 0: the maximum, its lowest index, and whether anything is finite
  qqq_u64 best = 0ull;
  int finite = 0;
  for (int v = tid; v < nvec; v += SMP_NT) {
    const v4u x = qqq_sample_load(row, v, vocab);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned key = qqq_sample_key(qqq_sample_bits(x, e));
      const qqq_u64 cand = ((qqq_u64)key << 32) | (qqq_u64)(0xffffffffu - (unsigned)(8 * v + e));
      best = cand > best ? cand : best;
      finite |= (key >= 0x0400u && key <= 0xfbffu) ? 1 : 0;
    }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const qqq_u64 y = __shfl_xor(best, o);
    best = y > best ? y : best;
  }
  if (lane == 0) red[w] = best;
  finite = __syncthreads_or(finite);
#pragma unroll
  for (int i = 0; i < SMP_WAVES; ++i) best = red[i] > best ? red[i] : best;
  const unsigned kmax = (unsigned)(best >> 32);
  const long long imax = (long long)(0xffffffffu - (unsigned)(best & 0xffffffffull));
  if (!finite) {
    if (tid == 0) emit(r, 0ll);
    return;
  }
  if (!(T > 0.f) || k == 1) {
    if (tid == 0) emit(r, imax);
    return;
  }
  const bool topk = k > 1 && k < vocab;
  const bool topp = p < 1.f;
  const float lmax = qqq_sample_value(kmax);
  const float c = 1.4426950408889634f / T;
  unsigned kk = 0u, kp = 0u;

  if (topk || topp) {
    for (int i = tid; i < 256 * SMP_COPIES; i += SMP_NT) {
      hc[i] = 0u;
      hm[i] = 0ull;
    }
    __syncthreads();
    qqq_sample_hist<false>(row, vocab, nvec, 0u, topk, topp, kmax, lmax, c, hc, hm, tid);
    __syncthreads();
    if (tid < 256) {
      qqq_u64 a = 0ull, b = 0ull;
#pragma unroll
      for (int i = 0; i < SMP_COPIES; ++i) {
        a += hc[tid * SMP_COPIES + i];
        b += hm[tid * SMP_COPIES + i];
      }
      cnt[tid] = a;
      m1[tid] = b;
    }
    __syncthreads();
    int b1k = -1;
    if (topk) {
      qqq_u64 above;
      b1k = qqq_sample_select(cnt, (qqq_u64)k, above, lane);
      const qqq_u64 need2 = (qqq_u64)k - above;
      __syncthreads();  // cnt has been read by every wave
      for (int i = tid; i < 256 * SMP_COPIES; i += SMP_NT) {
        hc[i] = 0u;
        hm[i] = 0ull;
      }
      __syncthreads();
      qqq_sample_hist<true>(row, vocab, nvec, (unsigned)b1k, true, topp, kmax, lmax, c, hc, hm, tid);
      __syncthreads();
      if (tid < 256) {
        qqq_u64 a = 0ull, b = 0ull;
#pragma unroll
        for (int i = 0; i < SMP_COPIES; ++i) {
          a += hc[tid * SMP_COPIES + i];
          b += hm[tid * SMP_COPIES + i];
        }
        cnt[tid] = a;
        m2[tid] = b;
      }
      __syncthreads();
      const int lowk = qqq_sample_select(cnt, need2, above, lane);
      kk = ((unsigned)b1k << 8) | (unsigned)lowk;
      if (topp) {  // the masses of the kept keys alone: nothing below the top-k cut
        if (tid < lowk) m2[tid] = 0ull;
        __syncthreads();
        const qqq_u64 kept = qqq_sample_total(m2, lane);
        if (tid < 256) m1[tid] = tid < b1k ? 0ull : (tid == b1k ? kept : m1[tid]);
        __syncthreads();
      }
    }
    if (topp) {
      const qqq_u64 W = qqq_sample_total(m1, lane);
      qqq_u64 need = 1ull;  // p <= 0: the maximum's tie group alone
      if (p > 0.f) {
        const qqq_u64 thr = (qqq_u64)((1.0 - (double)p) * (double)W);
        need = thr < W ? W - thr : 1ull;
      }
      qqq_u64 above;
      const int b1p = qqq_sample_select(m1, need, above, lane);
      const qqq_u64 need2 = need - above;
      if (b1p != b1k) {
        __syncthreads();
        for (int i = tid; i < 256 * SMP_COPIES; i += SMP_NT) hm[i] = 0ull;
        __syncthreads();
        qqq_sample_hist<true>(row, vocab, nvec, (unsigned)b1p, false, true, kmax, lmax, c, hc, hm, tid);
        __syncthreads();
        if (tid < 256) {
          qqq_u64 b = 0ull;
#pragma unroll
          for (int i = 0; i < SMP_COPIES; ++i) b += hm[tid * SMP_COPIES + i];
          m2[tid] = b;
        }
        __syncthreads();
      }
      const int lowp = qqq_sample_select(m2, need2, above, lane);
      kp = ((unsigned)b1p << 8) | (unsigned)lowp;
    }
  }
  unsigned ks = kk > kp ? kk : kp;
  ks = ks > 1u ? ks : 1u;

  // ---- the draw: wave w owns the vectors [w * seg, (w + 1) * seg) in token order
  const int seg = (nvec + SMP_WAVES - 1) / SMP_WAVES;
  const int steps = (seg + 63) >> 6;
  const int v0 = w * seg;
  qqq_u64 mine = 0ull;
  for (int i = 0; i < steps; ++i) {
    const int o = 64 * i + lane, v = v0 + o;
    if (o < seg && v < nvec) {
      const v4u x = qqq_sample_load(row, v, vocab);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned b = qqq_sample_bits(x, e);
        mine += qqq_sample_weight(b, qqq_sample_key(b), ks, kmax, lmax, c);
      }
    }
  }
  mine = qqq_sample_wave_sum(mine);
  __syncthreads();  // red was read in walk 0
  if (lane == 0) red[w] = mine;
  __syncthreads();
  qqq_u64 W2 = 0ull;
#pragma unroll
  for (int i = 0; i < SMP_WAVES; ++i) W2 += red[i];
  float uc = u >= 0.f ? u : 0.f;  // NaN and negatives to 0
  uc = uc < 1.f ? uc : 0.99999994f;
  qqq_u64 target = (qqq_u64)((double)uc * (double)W2);
  target = target < W2 ? target : W2 - 1ull;  // W2 >= 2^44: the maximum survives both cuts
  qqq_u64 base = 0ull;
  int hw = SMP_WAVES - 1;
  {
    qqq_u64 run = 0ull;
    bool found = false;
#pragma unroll
    for (int i = 0; i < SMP_WAVES; ++i) {
      if (!found && run + red[i] > target) {
        hw = i;
        base = run;
        found = true;
      }
      run += red[i];
    }
  }
  if (w != hw) return;
  qqq_u64 run = base;
  for (int i = 0; i < steps; ++i) {
    const int o = 64 * i + lane, v = v0 + o;
    qqq_u64 f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = 0ull;
    if (o < seg && v < nvec) {
      const v4u x = qqq_sample_load(row, v, vocab);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned b = qqq_sample_bits(x, e);
        f[e] = qqq_sample_weight(b, qqq_sample_key(b), ks, kmax, lmax, c);
      }
    }
    qqq_u64 s = 0ull;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += f[e];
    const qqq_u64 incl = qqq_sample_wave_scan(s, lane);
    const qqq_u64 tot = __shfl(incl, 63);
    if (run + tot > target) {  // wave-uniform
      const qqq_u64 hit = __ballot(run + incl > target);
      if (lane == __ffsll((long long)hit) - 1) {
        qqq_u64 acc = run + incl - s;
        int tok = -1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          acc += f[e];
          if (tok < 0 && acc > target) tok = 8 * v + e;
        }
        emit(r, (long long)tok);
      }
      return;
    }
    run += tot;
  }
  if (lane == 0) emit(r, imax);  // not reached: the sums are exact, so the owning wave finds its token
}

__global__ __launch_bounds__(SMP_NT) void qqq_sample_tokens_kernel(const unsigned short* __restrict__ logits, const int ld,
                                                                   const float* __restrict__ temperature, const int* __restrict__ top_k,
                                                                   const float* __restrict__ top_p, const float* __restrict__ uu,
                                                                   long long* __restrict__ tokens, const int vocab) {
  qqq_sample_row(logits, ld, temperature, top_k, top_p, vocab, blockIdx.x, qqq_sample_store{uu, tokens});
}

#endif  // QQQ_AMD_QQQ_SAMPLE_HIP_H_
