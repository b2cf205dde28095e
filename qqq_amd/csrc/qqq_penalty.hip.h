// qqq_penalty.hip.h -- the repetition / presence / frequency penalty (include/qqq_amd_penalty.h): the fp16 logits of a batch rewritten in
// place, conditioned on the tokens each row has seen, in ONE launch in front of a sampler.  Part of the single translation unit qqq_w4a8.hip.
//
//   qqq_penalize_logits_kernel   One workgroup (16 waves) per row; the work is O(history + group) per row, not O(vocab).
//     walk          the row's "walk" is its history seen[r, 0 ... p] -- index p taken from ids[r, 0], which lane 0 also records there --
//                   followed by its drafts ids[r, 1 ... G-1] at the indices p + 1 ... p + G - 1; lane `tid` takes the indices tid,
//                   tid + 1024, ...  Tokens outside [0, vocab) are skipped.
//     scatter       every index of the walk marks its token's word of the row's workspace (zero on entry) with one integer atomic:
//                   OR of bit 31 for a prompt index, ADD of 1 for an output index, OR of bit 30 for a draft.  Nothing is returned.
//     barrier       every wave drains its atomics (s_waitcnt vmcnt(0)) and the workgroup meets: the words are final.
//     collect       the same walk again, each index swapping 0 into its token's word: of all the indices that name a token exactly one
//                   receives the non-zero word -- it owns the token -- and the word is zero again for the next call.  The owner applies
//                   the rule to the token's entry of each of the row's G logits rows: row j takes the history's counts plus what the
//                   drafts 1 ... j add (a draft is an output occurrence iff its index p + k is no prompt index), and a token that only
//                   the drafts name is touched from the row of its first draft on.  One lane per token and logits row: no entry is
//                   read or written twice, and what is applied depends on the final words alone, not on the arrival order.
//   Every access to the workspace is an atomic (performed at the L2), so no wave ever reads a workspace word through its L1; the logits
//   entries and seen[r, p] are touched by one lane each.  The output count of a token stays below bit 30: seen_stride < 2^30.
#ifndef QQQ_AMD_QQQ_PENALTY_HIP_H_
#define QQQ_AMD_QQQ_PENALTY_HIP_H_

static constexpr int PEN_NT = 1024;
static constexpr int PEN_MAX_GROUP = 16;
static constexpr int PEN_MAX_SEEN = (1 << 30) - 1;  // seen_stride: an output count never reaches bit 30
static constexpr unsigned PEN_PROMPT = 0x80000000u, PEN_DRAFT = 0x40000000u, PEN_COUNT = 0x3fffffffu;

// The rule on one logit with c output occurrences: each line one correctly rounded f32 operation, never contracted into an FMA.
__device__ __forceinline__ unsigned short qqq_penalty_rule(const unsigned short b, const unsigned c, const float rep, const float pres,
                                                           const float freq) {
#pragma clang fp contract(off)
  float x = (float)__builtin_bit_cast(_Float16, b);
  if (rep != 1.f) x = x > 0.f ? __fdiv_rn(x, rep) : x * rep;
  if (c > 0u) {
    const float f = freq * (float)c;
    x = x - f;
    x = x - pres;
  }
  return __builtin_bit_cast(unsigned short, (_Float16)x);
}

__global__ __launch_bounds__(PEN_NT) void qqq_penalize_logits_kernel(unsigned short* __restrict__ logits, const int ld,
                                                                     const long long* __restrict__ ids, const long long* __restrict__ pos,
                                                                     const int group, int* __restrict__ seen, const int seen_stride,
                                                                     const int* __restrict__ n_prompt, const float* __restrict__ repetition,
                                                                     const float* __restrict__ presence, const float* __restrict__ frequency,
                                                                     unsigned* __restrict__ ws, const int vocab) {
  __shared__ int draft[PEN_MAX_GROUP];  // draft[k], k >= 1: ids[r, k] if in [0, vocab), else -1

  const int r = blockIdx.x, tid = threadIdx.x;
  const long long* rid = ids + (size_t)r * group;
  const long long p64 = pos[(size_t)r * group];
  if (p64 < 0 || p64 >= (long long)seen_stride) return;  // idle, or a position the history cannot hold: nothing is read or written
  const int p = (int)p64;
  const long long id0 = rid[0];
  const int rec = (id0 >= 0 && id0 < (long long)vocab) ? (int)id0 : -1;
  int* hist = seen + (size_t)r * seen_stride;
  if (tid == 0) hist[p] = rec;
  const float rep = repetition[r], pres = presence[r], freq = frequency[r];
  if (rep == 1.f && pres == 0.f && freq == 0.f) return;  // neutral: recorded, no logits row written (row-uniform: no barrier is skipped by a part)
  const int np = n_prompt[r];
  if (tid >= 1 && tid < group) {
    const long long d = rid[tid];
    draft[tid] = (d >= 0 && d < (long long)vocab) ? (int)d : -1;
  }
  __syncthreads();
  unsigned* W = ws + (size_t)r * vocab;
  const int n = p + group;  // p < 2^30, group <= 16

  for (int i = tid; i < n; i += PEN_NT) {
    const int t = i < p ? hist[i] : (i == p ? rec : draft[i - p]);
    if (t < 0 || t >= vocab) continue;
    if (i > p)
      atomicOr(&W[t], PEN_DRAFT);
    else if (i < np)
      atomicOr(&W[t], PEN_PROMPT);
    else
      atomicAdd(&W[t], 1u);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's atomics have been performed
  __syncthreads();

  for (int i = tid; i < n; i += PEN_NT) {
    const int t = i < p ? hist[i] : (i == p ? rec : draft[i - p]);
    if (t < 0 || t >= vocab) continue;
    const unsigned v = atomicExch(&W[t], 0u);
    if (v == 0u) continue;  // another index owns the token
    bool present = (v & ~PEN_DRAFT) != 0u;  // in the history
    unsigned c = v & PEN_COUNT;
    unsigned short* l = logits + (size_t)r * group * ld + t;
    for (int j = 0; j < group; ++j, l += ld) {
      if (j > 0 && draft[j] == t) {
        present = true;
        c += (p + j >= np) ? 1u : 0u;
      }
      if (present) *l = qqq_penalty_rule(*l, c, rep, pres, freq);
    }
  }
}

#endif  // QQQ_AMD_QQQ_PENALTY_HIP_H_
