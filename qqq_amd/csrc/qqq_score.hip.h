// qqq_score.hip.h -- the fused scoring kernel (include/qqq_amd_score.h): the log-probability of one target token per row of a batch of fp16
// logits, and the row's argmax, in ONE launch.  Part of the single translation unit qqq_w4a8.hip, behind qqq_sample.hip.h, whose key
// order, fixed-point weights and row loads it reuses: a row's W is the sampler's W at T = 1, to the bit.
//
//   qqq_token_logprobs_kernel  One workgroup (16 waves) per row; the row is walked twice (the first walk from HBM or wherever the head GEMM
//                              left it, the second from the L2), 16 bytes per lane and instruction, two loads in flight per lane, the
//                              vocab % 8 tail by scalar loads: the padding columns vocab ... ld - 1 are never read.
//     walk 0        the maximum key and its lowest index: the sampler's 64-bit max over key << 32 | ~index.
//     walk 1        W = the sum of the fixed-point weights (qqq_sample_weight with no cut and c = log2 e): 64-bit integers, so the sum is
//                   exact whatever the order -- per lane, then a wave reduction, then sixteen partial sums through LDS.
//     result        one lane: ((double)l_t - (double)l_max) - log((double)W * 2^-44), rounded to f32 once.
//   A target outside [0, vocab) needs no W: walk 1 is skipped, and walk 0 too when no argmax is asked for.
#ifndef QQQ_AMD_QQQ_SCORE_HIP_H_
#define QQQ_AMD_QQQ_SCORE_HIP_H_

static constexpr int SCR_UNROLL = 2;  // 16-byte loads in flight per lane in the body of a walk (57 registers: two workgroups per CU; 4 spills SGPRs)

// the walk of one row: f(x, v) for every vector v of eight tokens, each exactly once, SCR_UNROLL loads issued ahead of their use; the
// vector that holds the vocab % 8 tail goes through qqq_sample_load (scalar loads, nothing read from `vocab` on)
template <class F>
__device__ __forceinline__ void qqq_score_walk(const unsigned short* __restrict__ row, const int vocab, const int tid, F f) {
  const int nfull = vocab >> 3;
  int v = tid;
  for (; v + (SCR_UNROLL - 1) * SMP_NT < nfull; v += SCR_UNROLL * SMP_NT) {
    v4u x[SCR_UNROLL];
#pragma unroll
    for (int i = 0; i < SCR_UNROLL; ++i) x[i] = *reinterpret_cast<const v4u*>(row + 8 * (v + i * SMP_NT));
#pragma unroll
    for (int i = 0; i < SCR_UNROLL; ++i) f(x[i], v + i * SMP_NT);
  }
  for (; v < nfull; v += SMP_NT) f(*reinterpret_cast<const v4u*>(row + 8 * v), v);
  if ((vocab & 7) && v == nfull) f(qqq_sample_load(row, nfull, vocab), nfull);  // elements from `vocab` on come back as NaN: key 0
}

__global__ __launch_bounds__(SMP_NT) void qqq_token_logprobs_kernel(const unsigned short* __restrict__ logits, const int ld,
                                                                    const long long* __restrict__ targets, float* __restrict__ logprob,
                                                                    long long* __restrict__ argmax, const int vocab) {
  __shared__ qqq_u64 red[SMP_WAVES];
  __shared__ qqq_u64 sum[SMP_WAVES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = blockIdx.x;
  const unsigned short* row = logits + (size_t)r * ld;
  const long long t = targets[r];
  const bool scored = t >= 0 && t < (long long)vocab;
  if (!scored && !argmax) {  // nothing of the row is needed
    if (tid == 0) logprob[r] = t < 0 ? 0.f : __builtin_nanf("");
    return;
  }

  // ---- walk 0: the maximum and its lowest index
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
  __syncthreads();
#pragma unroll
  for (int i = 0; i < SMP_WAVES; ++i) best = red[i] > best ? red[i] : best;
  const unsigned kmax = (unsigned)(best >> 32);
  const long long imax = kmax ? (long long)(0xffffffffu - (unsigned)(best & 0xffffffffull)) : 0ll;  // nothing above -inf: 0
  if (tid == 0 && argmax) argmax[r] = imax;
  if (!scored || kmax == 0u) {
    if (tid == 0) logprob[r] = t < 0 ? 0.f : __builtin_nanf("");
    return;
  }

  // ---- walk 1: W, the sampler's weights at T = 1 without a cut
  const float lmax = qqq_sample_value(kmax);
  const float c = 1.4426950408889634f;  // the sampler's 1.4426950408889634f / T at T = 1
  qqq_u64 mine = 0ull;
  qqq_score_walk(row, vocab, tid, [&](const v4u x, const int) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned b = qqq_sample_bits(x, e);
      mine += qqq_sample_weight(b, qqq_sample_key(b), 1u, kmax, lmax, c);
    }
  });
  mine = qqq_sample_wave_sum(mine);
  if (lane == 0) sum[w] = mine;
  __syncthreads();
  if (tid != 0) return;
  qqq_u64 W = 0ull;
#pragma unroll
  for (int i = 0; i < SMP_WAVES; ++i) W += sum[i];  // >= 2^44: the maximum itself
  const unsigned bt = row[t];
  const unsigned kt = qqq_sample_key(bt);
  float out;
  if (kt == 0u) {
    out = -__builtin_inff();  // NaN or -inf at the target: no weight
  } else {
    const double d = kt == kmax ? 0.0 : (double)qqq_sample_value(kt) - (double)lmax;  // -inf under a +inf maximum
    out = (float)(d - log((double)W * 0x1p-44));
  }
  logprob[r] = out;
}

#endif  // QQQ_AMD_QQQ_SCORE_HIP_H_
