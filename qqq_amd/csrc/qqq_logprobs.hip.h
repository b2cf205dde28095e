// qqq_logprobs.hip.h -- the fused top-k log-probability kernel (include/qqq_amd_logprobs.h): for every row of a batch of fp16 logits
// the log-probability and the rank of ONE token, and the k most probable tokens with their log-probabilities, in ONE launch.  Part of the
// single translation unit qqq_w4a8.hip, behind qqq_score.hip.h: the key order, the fixed-point weights and the radix select are the
// sampler's, the row walk the scorer's, and a value is the scorer's to the bit.
//
//   qqq_logprobs_row           One workgroup (16 waves) per row, shared by the two kernels below.
//     walk 0        the maximum key (the scorer's walk 0).  A row without a logit above -inf ends here: every value NaN, ids 0 ... k - 1.
//     walk 1        W (the scorer's walk 1), the number of keys above the token's (its rank - 1), and -- with k > 0 -- the counts of the
//                   key's high byte: the sampler's histogram copies in LDS.
//     walk 2        k > 0: the counts of the low byte inside the chosen bin (qqq_sample_hist<true>).  Two qqq_sample_select give tau, the
//                   k-th largest key, and how many keys lie above it: n_above < k.  The other k - n_above entries are the LOWEST indices
//                   among the keys equal to tau.
//     walk A        in token order, each wave a contiguous sixteenth of the row (the sampler's draw): the keys above tau go into an LDS
//                   list through an LDS counter, the keys equal to tau are counted per wave.
//     walk B        the waves whose ties can still make the cut go over their part again: a wave prefix, a lane scan, and a tie's place
//                   among the ties is its place in the list, until k - n_above are placed.
//     sort          one wave ranks the k words key << 32 | ~index against each other (all distinct) and writes them out in that order.
//   With k == 0 the kernel ends behind walk 1: the scorer plus the rank.
//   qqq_topk_kernel            the plain entry's: a row per workgroup;  qqq_topk_step_kernel  the decode loop's epilogue (see there)
#ifndef QQQ_AMD_QQQ_LOGPROBS_HIP_H_
#define QQQ_AMD_QQQ_LOGPROBS_HIP_H_

static constexpr int LGP_MAX_K = 32;

// the scorer's result for a token of key `kt` in a row of maximum key `kmax` (value lmax) and lse = log(W * 2^-44), in its operations
__device__ __forceinline__ float qqq_logprobs_value(const unsigned kt, const unsigned kmax, const float lmax, const double lse) {
  if (kmax == 0u) return __builtin_nanf("");  // no logit above -inf
  if (kt == 0u) return -__builtin_inff();     // NaN or -inf at the token: no weight
  const double d = kt == kmax ? 0.0 : (double)qqq_sample_value(kt) - (double)lmax;  // -inf under a +inf maximum
  return (float)(d - lse);
}

__device__ __forceinline__ unsigned qqq_logprobs_wave_sum(unsigned x) {
#pragma unroll
  for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// One row by one workgroup.  has_t: a token `t` is scored into *lp and *rk; k > 0: top_ids[0 ... k-1] and top_lp[0 ... k-1] are written.
// Every lane of the workgroup calls it with the same arguments.
__device__ __forceinline__ void qqq_logprobs_row(const unsigned short* __restrict__ row, const int vocab, const bool has_t, const long long t,
                                                 const int k, float* __restrict__ lp, int* __restrict__ rk, int* __restrict__ top_ids,
                                                 float* __restrict__ top_lp) {
  __shared__ unsigned hc[256 * SMP_COPIES];
  __shared__ qqq_u64 cnt[256];
  __shared__ qqq_u64 red[SMP_WAVES];
  __shared__ qqq_u64 sum[SMP_WAVES];
  __shared__ unsigned gtw[SMP_WAVES];
  __shared__ unsigned tw[SMP_WAVES];
  __shared__ qqq_u64 list[LGP_MAX_K];
  __shared__ unsigned nlist;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool scored = has_t && t >= 0 && t < (long long)vocab;
  if (k == 0 && !scored) {  // nothing of the row is needed
    if (tid == 0 && has_t) {
      *lp = t < 0 ? 0.f : __builtin_nanf("");
      *rk = 0;
    }
    return;
  }

  // ---- walk 0: the maximum key
  qqq_u64 best = 0ull;
  qqq_score_walk(row, vocab, tid, [&](const v4u x, const int v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned key = qqq_sample_key(qqq_sample_bits(x, e));
      const qqq_u64 cand = ((qqq_u64)key << 32) | (qqq_u64)(0xffffffffu - (unsigned)(8 * v + e));
      best = cand > best ? cand : best;
    }
  });
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const qqq_u64 y = __shfl_xor(best, o);
    best = y > best ? y : best;
  }
  if (lane == 0) red[w] = best;
  if (tid == 0) nlist = 0u;
  for (int i = tid; i < 256 * SMP_COPIES; i += SMP_NT) hc[i] = 0u;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < SMP_WAVES; ++i) best = red[i] > best ? red[i] : best;
  const unsigned kmax = (unsigned)(best >> 32);
  if (kmax == 0u) {  // every key is 0: the order is the index order, and no value exists
    if (tid == 0 && has_t) {
      *lp = t < 0 ? 0.f : __builtin_nanf("");
      *rk = scored ? 1 : 0;
    }
    if (tid < k) {
      top_ids[tid] = tid;
      top_lp[tid] = __builtin_nanf("");
    }
    return;
  }

  // ---- walk 1: W, the keys above the token's, the counts of the high byte
  const float lmax = qqq_sample_value(kmax);
  const float c = 1.4426950408889634f;  // the scorer's: the sampler's log2 e / T at T = 1
  const unsigned kt = scored ? qqq_sample_key((unsigned)row[t]) : 0xffffffffu;
  const int cp = tid & (SMP_COPIES - 1);
  qqq_u64 mine = 0ull;
  unsigned gt = 0u;
  qqq_score_walk(row, vocab, tid, [&](const v4u x, const int v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned b = qqq_sample_bits(x, e);
      const unsigned key = qqq_sample_key(b);
      mine += qqq_sample_weight(b, key, 1u, kmax, lmax, c);
      gt += key > kt ? 1u : 0u;  // an element from `vocab` on has key 0
      if (k > 0) atomicAdd(&hc[(int)(key >> 8) * SMP_COPIES + cp], 1u);  // ... and is counted in bin 0: taken out below
    }
  });
  mine = qqq_sample_wave_sum(mine);
  gt = qqq_logprobs_wave_sum(gt);
  if (lane == 0) {
    sum[w] = mine;
    gtw[w] = gt;
  }
  __syncthreads();
  double lse = 0.0;
  if (w == 0) {  // the one wave that writes values
    qqq_u64 W = 0ull;
#pragma unroll
    for (int i = 0; i < SMP_WAVES; ++i) W += sum[i];  // >= 2^44: the maximum itself
    lse = log((double)W * 0x1p-44);
    if (tid == 0 && has_t) {
      unsigned above = 0u;
#pragma unroll
      for (int i = 0; i < SMP_WAVES; ++i) above += gtw[i];
      *lp = scored ? qqq_logprobs_value(kt, kmax, lmax, lse) : (t < 0 ? 0.f : __builtin_nanf(""));
      *rk = scored ? (int)(above + 1u) : 0;
    }
  }
  if (k == 0) return;

  // ---- the threshold key tau: the high byte from walk 1's counts, the low byte from a walk of its own
  if (tid < 256) {
    qqq_u64 a = 0ull;
#pragma unroll
    for (int i = 0; i < SMP_COPIES; ++i) a += hc[tid * SMP_COPIES + i];
    cnt[tid] = tid ? a : a - (qqq_u64)(-vocab & 7);  // without the elements from `vocab` on that the tail vector brought
  }
  __syncthreads();
  qqq_u64 above1, above2;
  const int b1 = qqq_sample_select(cnt, (qqq_u64)k, above1, lane);  // the counts hold every token: the total is vocab >= k
  const qqq_u64 need2 = (qqq_u64)k - above1;
  for (int i = tid; i < 256 * SMP_COPIES; i += SMP_NT) hc[i] = 0u;  // every hc was read in front of the barrier above
  __syncthreads();                                                  // ... and cnt by every wave
  const int nvec = (vocab + 7) >> 3;
  qqq_sample_hist<true>(row, vocab, nvec, (unsigned)b1, true, false, kmax, lmax, c, hc, nullptr, tid);
  __syncthreads();
  if (tid < 256) {
    qqq_u64 a = 0ull;
#pragma unroll
    for (int i = 0; i < SMP_COPIES; ++i) a += hc[tid * SMP_COPIES + i];
    cnt[tid] = a;
  }
  __syncthreads();
  const int low = qqq_sample_select(cnt, need2, above2, lane);
  const unsigned tau = ((unsigned)b1 << 8) | (unsigned)low;
  const unsigned n_above = (unsigned)(above1 + above2);  // < k
  const unsigned n_take = (unsigned)k - n_above;         // >= 1, and at most the number of keys equal to tau

  // ---- walk A: wave w owns the vectors [w * seg, (w + 1) * seg) in token order
  const int seg = (nvec + SMP_WAVES - 1) / SMP_WAVES;
  const int steps = (seg + 63) >> 6;
  const int v0 = w * seg;
  unsigned ties = 0u;
  for (int i = 0; i < steps; ++i) {
    const int o = 64 * i + lane, v = v0 + o;
    if (o < seg && v < nvec) {
      const v4u x = qqq_sample_load(row, v, vocab);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (8 * v + e >= vocab) continue;
        const unsigned key = qqq_sample_key(qqq_sample_bits(x, e));
        if (key > tau) {
          const unsigned slot = atomicAdd(&nlist, 1u);
          if (slot < (unsigned)LGP_MAX_K) list[slot] = ((qqq_u64)key << 32) | (qqq_u64)(0xffffffffu - (unsigned)(8 * v + e));
        }
        ties += key == tau ? 1u : 0u;
      }
    }
  }
  ties = qqq_logprobs_wave_sum(ties);
  if (lane == 0) tw[w] = ties;
  __syncthreads();

  // ---- walk B: the first n_take ties in token order
  unsigned run = 0u;
#pragma unroll
  for (int i = 0; i < SMP_WAVES; ++i) run += i < w ? tw[i] : 0u;
  if (run < n_take) {  // wave-uniform
    for (int i = 0; i < steps; ++i) {
      const int o = 64 * i + lane, v = v0 + o;
      unsigned m = 0u;  // which of the vector's eight tokens tie
      if (o < seg && v < nvec) {
        const v4u x = qqq_sample_load(row, v, vocab);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (8 * v + e < vocab && qqq_sample_key(qqq_sample_bits(x, e)) == tau) m |= 1u << e;
      }
      const unsigned n = (unsigned)__popc(m);
      unsigned incl = n;
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const unsigned y = __shfl_up(incl, s);
        if (lane >= s) incl += y;
      }
      unsigned ord = run + incl - n;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (m & (1u << e)) {
          if (ord < n_take && n_above + ord < (unsigned)LGP_MAX_K) list[n_above + ord] =((qqq_u64)tau << 32) | (qqq_u64)(0xffffffffu - (unsigned)(8 * v + e));  // n_above + ord < k
          ++ord;
        }
      run += __shfl(incl, 63);
      if (run >= n_take) break;
    }
  }
  __syncthreads();

  // ---- the sort: k distinct words, each lane counts the larger ones
  if (w != 0) return;
  const qqq_u64 x = lane < k ? list[lane] : 0ull;
  int place = 0;
#pragma unroll
  for (int j = 0; j < LGP_MAX_K; ++j) {
    const qqq_u64 y = __shfl(x, j);
    place += (j < k && y > x) ? 1 : 0;
  }
  if (lane < k) {
    top_ids[place] = (int)(0xffffffffu - (unsigned)(x & 0xffffffffull));
    top_lp[place] = qqq_logprobs_value((unsigned)(x >> 32), kmax, lmax, lse);
  }
}

__global__ __launch_bounds__(SMP_NT) void qqq_topk_kernel(const unsigned short* __restrict__ logits, const int ld,
                                                                   const long long* __restrict__ tokens, float* __restrict__ logprob,
                                                                   int* __restrict__ rank, int* __restrict__ top_ids,
                                                                   float* __restrict__ top_lp, const int k, const int vocab) {
  const int r = blockIdx.x;
  const bool has_t = tokens != nullptr;
  qqq_logprobs_row(logits + (size_t)r * ld, vocab, has_t, has_t ? tokens[r] : -1ll, k, has_t ? logprob + r : nullptr,
                   has_t ? rank + r : nullptr, k ? top_ids + (size_t)r * k : nullptr, k ? top_lp + (size_t)r * k : nullptr);
}

// The decode loop's epilogue behind qqq_sample_advance: a row that holds a token without a record yet (n_rec < n_out) scores the logits
// row it was drawn from into record n_rec and counts it.  The workgroup reads n_rec[r] in front of a barrier and one lane writes it behind.
__global__ __launch_bounds__(SMP_NT) void qqq_topk_step_kernel(const unsigned short* __restrict__ logits, const int ld,
                                                                        const long long* __restrict__ out, const int out_stride,
                                                                        const int* __restrict__ n_out, int* __restrict__ n_rec,
                                                                        float* __restrict__ logprob, int* __restrict__ rank,
                                                                        int* __restrict__ top_ids, float* __restrict__ top_lp, const int cap,
                                                                        const int k, const int vocab) {
  const int r = blockIdx.x;
  const int a = n_rec[r];
  const int b = n_out[r];
  __syncthreads();
  if (a < 0 || a >= b || a >= cap || a >= out_stride) return;  // idle, nothing new this step, or no room
  const size_t rec = (size_t)r * cap + a;
  qqq_logprobs_row(logits + (size_t)r * ld, vocab, true, out[(size_t)r * out_stride + a], k, logprob + rec, rank + rec,
                   k ? top_ids + rec * k : nullptr, k ? top_lp + rec * k : nullptr);
  if (threadIdx.x == 0) n_rec[r] = a + 1;
}

#endif  // QQQ_AMD_QQQ_LOGPROBS_HIP_H_
