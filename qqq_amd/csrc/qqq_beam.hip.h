// qqq_beam.hip.h -- beam search on the device (include/qqq_amd_beam.h): the step behind a pass's logits and the block copies of a
// cache reorder.  Part of the single translation unit qqq_w4a8.hip, behind qqq_logprobs.hip.h, whose row body it calls: key order,
// fixed-point weights, radix select and the scorer's logarithm are that header's device functions, not copies of them.
//
//   qqq_beam_rows_kernel    One workgroup (16 waves) per logits row p * B + b.  A live row runs qqq_logprobs_row with k = 2B into the
//                           workspace: ids and log-probabilities of its 2B candidates, in that op's order.  A dead row writes nothing.
//   qqq_beam_merge_kernel   Behind it on the stream: one wave per prompt (4 per workgroup).  The B rows' candidate lists are sorted
//                           already (a row's scores are cum + lp with one cum, and f32 addition is monotonic), so 2B rounds of "the best
//                           head of B lists" order the prompt's first 2B candidates: the word key(score) << 32 | ~(b * 2B + i) is
//                           distinct per candidate and its order is (score descending, b ascending, i ascending).  Lane b < B keeps
//                           list b's head, lane j < 2B ends up with candidate j and writes cand_*[p, j]; a ballot over "token is not eos"
//                           gives the non-eos candidates their places, and the first B of them become the next beams.
//                           Every index into the workspace is below B * 2B by construction (it is a lane's list position).
//   Two launches and a workspace, no host sync: a merge inside the first launch (a ticket per prompt, the last row to arrive merges) was
//   built first and keeps eight output pointers live across the row body -- 29 SGPRs spilled; the second launch costs less than that.
//   qqq_copy_blocks_kernel  workgroup (j, pool): block src[j] -> block dst[j] of that pool, 16 bytes per lane and trip.  Block ids outside
//                           [0, num_blocks) and a pool base that is not 16-byte aligned copy nothing.
#ifndef QQQ_AMD_QQQ_BEAM_HIP_H_
#define QQQ_AMD_QQQ_BEAM_HIP_H_

static constexpr int BEAM_MAX = 16;  // beams per prompt: k = 2B <= LGP_MAX_K
static constexpr int BEAM_NT = 256;
static constexpr int BEAM_WAVES = BEAM_NT / 64;
static constexpr int COPY_NT = 256;

static_assert(2 * BEAM_MAX <= LGP_MAX_K, "a row's 2B candidates come from the top-k row body");

__global__ __launch_bounds__(SMP_NT) void qqq_beam_rows_kernel(const unsigned short* __restrict__ logits, const int ld,
                                                                const int* __restrict__ live, int* __restrict__ ws_ids,
                                                                float* __restrict__ ws_lp, const int k, const int vocab) {
  const int row = blockIdx.x;
  if (live[row] == 0) return;  // workgroup-uniform
  qqq_logprobs_row(logits + (size_t)row * ld, vocab, false, -1ll, k, nullptr, nullptr, ws_ids + (size_t)row * k, ws_lp + (size_t)row * k);
}

struct qqq_beam_args {
  const float* cum;
  const int* live;
  const int* ws_ids;   // int32 [P * B, 2B]: the rows' candidates
  const float* ws_lp;  // f32 [P * B, 2B]
  float* cand_score;
  float* cand_logprob;
  int* cand_parent;
  int* cand_token;
  long long* next_ids;
  int* next_parent;
  float* next_cum;
  int* next_live;
  int B, eos, prompts;
};

// what the merge compares: NaN and -inf are 0 (equal, below everything), -0 equals +0, every other value keeps its order
__device__ __forceinline__ unsigned qqq_beam_key(const float s) {
  const unsigned u = __float_as_uint(s + 0.0f);
  if (s != s || u == 0xff800000u) return 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(BEAM_NT) void qqq_beam_merge_kernel(const qqq_beam_args a) {
  __shared__ qqq_u64 words[BEAM_WAVES][2 * BEAM_MAX * BEAM_MAX];
  const int w = threadIdx.x >> 6;
  const int p = blockIdx.x * BEAM_WAVES + w;
  const int lane = threadIdx.x & 63;
  const bool active = p < a.prompts;  // wave-uniform
  const int B = a.B, k = 2 * B;
  const int base = active ? p * B : 0;
  const float* lps = a.ws_lp + (size_t)base * k;
  const int* ids = a.ws_ids + (size_t)base * k;
  if (active)
    for (int t = lane; t < B * k; t += 64) {  // a dead row's candidates were never written and are never read
      const int r = base + t / k;
      words[w][t] = a.live[r] != 0 ? ((qqq_u64)qqq_beam_key(a.cum[r] + lps[t]) << 32) | (qqq_u64)(0xffffffffu - (unsigned)t) : 0ull;
    }
  __syncthreads();
  if (!active) return;
  int head = lane < B ? 0 : k;  // lanes 0 ... B - 1: the next candidate of row `lane`
  qqq_u64 mine = 0ull;          // lanes 0 ... 2B - 1: candidate `lane` of the prompt; 0: none
  for (int j = 0; j < k; ++j) {
    const qqq_u64 c = head < k ? words[w][lane * k + head] : 0ull;  // a dead row's head is 0 and is never taken
    qqq_u64 best = c;
#pragma unroll
    for (int o = BEAM_MAX / 2; o; o >>= 1) {
      const qqq_u64 y = __shfl_xor(best, o);
      best = y > best ? y : best;
    }
    best = __shfl(best, 0);
    if (best != 0ull && c == best) ++head;  // the words are distinct
    if (lane == j) mine = best;
  }
  const bool have = lane < k && mine != 0ull;  // a prompt with a live row has 2B candidates, a prompt without has none
  int tok = -1, par = -1;
  float lp = -__builtin_inff(), score = -__builtin_inff();
  if (have) {
    const int at = (int)(0xffffffffu - (unsigned)(mine & 0xffffffffull));  // b * 2B + i < B * 2B
    par = at / k;
    tok = ids[at];
    lp = lps[at];
    score = a.cum[base + par] + lp;
  }
  if (lane < k) {
    const size_t o = (size_t)p * k + lane;
    a.cand_score[o] = score;
    a.cand_logprob[o] = lp;
    a.cand_parent[o] = par;
    a.cand_token[o] = tok;
  }
  const bool goes_on = have && !(a.eos >= 0 && tok == a.eos);
  const unsigned long long mask = __ballot(goes_on);
  const int place = __popcll(mask & ((1ull << lane) - 1ull));
  if (goes_on && place < B) {
    const size_t o = (size_t)base + place;
    a.next_ids[o] = (long long)tok;
    a.next_parent[o] = par;
    a.next_cum[o] = score;
    a.next_live[o] = 1;
  }
  if (lane < B && lane >= __popcll(mask)) {  // a prompt without a live row: its rows stay dead
    const size_t o = (size_t)base + lane;
    a.next_ids[o] = 0ll;
    a.next_parent[o] = -1;
    a.next_cum[o] = -__builtin_inff();
    a.next_live[o] = 0;
  }
}

__global__ __launch_bounds__(COPY_NT) void qqq_copy_blocks_kernel(const void* const* __restrict__ pools, const int* __restrict__ src,
                                                                  const int* __restrict__ dst, const unsigned vecs, const int num_blocks) {
  const int s = src[blockIdx.x], d = dst[blockIdx.x];
  if (s < 0 || s >= num_blocks || d < 0 || d >= num_blocks || s == d) return;
  const char* pool = static_cast<const char*>(pools[blockIdx.y]);
  if (pool == nullptr || (reinterpret_cast<size_t>(pool) & 15u)) return;
  const v4u* from = reinterpret_cast<const v4u*>(pool) + (size_t)s * vecs;
  v4u* to = reinterpret_cast<v4u*>(const_cast<char*>(pool)) + (size_t)d * vecs;
  for (unsigned i = threadIdx.x; i < vecs; i += COPY_NT) to[i] = from[i];
}

#endif  // QQQ_AMD_QQQ_BEAM_HIP_H_
