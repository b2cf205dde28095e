// qqq_guided.hip.h -- guided decoding (include/qqq_amd_guided.h): a completion follows a token automaton held in device memory
// in CSR form.  Two integer kernels around a decode loop's sampler, both inside its captured step.  Part of the single translation unit
// qqq_w4a8.hip.
//
//   qqq_fsm_mask_kernel     grid (slices, rows): a workgroup owns `width` columns of one logits row (a multiple of 2048, at most 16384; the
//                           split is fsm_mask_width(rows, vocab)).  Every wave finds the slice's part of the state's ascending edge list by
//                           a 64-way search (64 probes per round, a ballot), the workgroup sets one bit per allowed column in an LDS bit
//                           set of the slice (2 KB), and then writes fp16 -inf around the set bits: a thread takes 8 columns at a time, one
//                           16-byte store where none of them is allowed and the address is 16-byte aligned, 2-byte stores otherwise.  The
//                           logits are never read.  A token is checked against the slice before it sets a bit, both offsets are clamped
//                           into [0, n_edges], and a search only probes inside them: whatever the arrays hold, nothing outside them or
//                           outside the row's [0, vocab) is touched.
//   qqq_fsm_advance_kernel  one wave per row (4 per workgroup): the tokens the row emitted since its state was last advanced are looked
//                           up in order by the same 64-way search; lane 0 writes the state, the count and a retiring row's ids / pos /
//                           slots / remaining.
#ifndef QQQ_AMD_QQQ_GUIDED_HIP_H_
#define QQQ_AMD_QQQ_GUIDED_HIP_H_

static constexpr int FSM_NT = 256;
static constexpr int FSM_WAVES = FSM_NT / 64;
static constexpr int FSM_PASS = FSM_NT * 8;        // columns a workgroup writes per pass: 8 per thread
static constexpr int FSM_MAX_WIDTH = 8 * FSM_PASS;  // columns of a slice: the LDS bit set holds one bit each
static constexpr int FSM_TARGET_GROUPS = 1024;     // workgroups a launch aims at when the rows are few

// the columns a workgroup owns: a function of (rows, vocab) alone
static inline int fsm_mask_width(const int rows, const int vocab) {
  const int most = (vocab + FSM_PASS - 1) / FSM_PASS, least = (vocab + FSM_MAX_WIDTH - 1) / FSM_MAX_WIDTH;
  int slices = (FSM_TARGET_GROUPS + rows - 1) / rows;
  slices = slices < least ? least : slices > most ? most : slices;
  const int share = (vocab + slices - 1) / slices;
  return (share + FSM_PASS - 1) / FSM_PASS * FSM_PASS;  // <= FSM_MAX_WIDTH: share <= ceil(vocab / least)
}

__device__ __forceinline__ int fsm_clamp(const int v, const int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// the first index in [lo, hi] whose token is >= key (hi: none), for ascending tokens[lo ... hi): 64 probes per round, by a whole wave.
// lo <= hi, both inside [0, n_edges]: every probe lies in [lo, hi).
__device__ __forceinline__ int fsm_lower_bound(const int* __restrict__ tokens, int lo, int hi, const int key, const int lane) {
  while (hi > lo) {  // wave-uniform
    const int step = (int)(((long long)hi - lo + 63) >> 6);
    const long long at = (long long)lo + (long long)lane * step;
    const bool below = at < (long long)hi && tokens[at] < key;
    const unsigned long long mask = ~__ballot(below);
    const int k = mask == 0ull ? 64 : __builtin_ctzll(mask);  // the probes in front of the first that is not below
    if (k == 0) break;
    const long long last = (long long)lo + (long long)(k - 1) * step;  // below the key; the probe behind it, if there is one, is not
    lo = (int)(last + 1);
    if (last + step < (long long)hi) hi = (int)(last + step);
  }
  return lo;
}

__global__ __launch_bounds__(FSM_NT) void qqq_fsm_mask_kernel(unsigned short* __restrict__ logits, const int ld, const int* __restrict__ state,
                                                              const int* __restrict__ eos, const int* __restrict__ remaining,
                                                              const int* __restrict__ offsets, const int* __restrict__ tokens,
                                                              const int* __restrict__ accept, const int n_states, const int n_edges,
                                                              const int vocab, const int width) {
  __shared__ unsigned bits[FSM_MAX_WIDTH / 32];
  const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int s = state[r];
  if (s < 0 || s >= n_states) return;                      // workgroup-uniform
  if (remaining != nullptr && remaining[r] == 0) return;  // an idle row
  const int c0 = blockIdx.x * width;
  if (c0 >= vocab) return;
  const int c1 = c0 + width < vocab ? c0 + width : vocab;  // the slice [c0, c1)
  const int lo = fsm_clamp(offsets[s], n_edges);
  int hi = fsm_clamp(offsets[s + 1], n_edges);
  if (hi < lo) hi = lo;
  for (int w = tid; w < width / 32; w += FSM_NT) bits[w] = 0u;
  const int a = fsm_lower_bound(tokens, lo, hi, c0, lane);
  const int b = fsm_lower_bound(tokens, a, hi, c1, lane);
  __syncthreads();
  for (int e = a + tid; e < b; e += FSM_NT) {
    const int t = tokens[e];
    if (t >= c0 && t < c1) atomicOr(&bits[(t - c0) >> 5], 1u << ((t - c0) & 31));
  }
  if (tid == 0 && eos != nullptr && accept[s] != 0) {
    const int t = eos[r];
    if (t >= c0 && t < c1) atomicOr(&bits[(t - c0) >> 5], 1u << ((t - c0) & 31));
  }
  __syncthreads();
  unsigned short* row = logits + (size_t)r * (size_t)ld;
  const uint4 ninf = make_uint4(0xFC00FC00u, 0xFC00FC00u, 0xFC00FC00u, 0xFC00FC00u);
  for (int g = tid; g < width / 8; g += FSM_NT) {
    const int c = c0 + 8 * g;
    if (c >= c1) break;
    const unsigned keep = (bits[g >> 2] >> (8 * (g & 3))) & 0xffu;
    unsigned short* p = row + c;
    if (keep == 0u && c + 8 <= c1 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      *reinterpret_cast<uint4*>(p) = ninf;
    } else {
      const int n = c1 - c < 8 ? c1 - c : 8;
      for (int j = 0; j < n; ++j)
        if (!((keep >> j) & 1u)) p[j] = (unsigned short)0xFC00u;
    }
  }
}

struct qqq_fsm_advance_args {
  const long long* out;
  const int* n_out;
  int* n_fsm;
  int* state;
  const int* eos;  // may be NULL
  const int* offsets;
  const int* tokens;
  const int* next;
  const int* accept;
  long long* ids;
  long long* pos;
  long long* slots;
  int* remaining;
  int out_stride, n_states, n_edges, rows;
};

__global__ __launch_bounds__(FSM_NT) void qqq_fsm_advance_kernel(const qqq_fsm_advance_args a) {
  const int r = blockIdx.x * FSM_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= a.rows) return;
  const int m = a.n_out[r], done = a.n_fsm[r];
  if (done >= m) return;  // wave-uniform: nothing new, nothing written
  const int eos = a.eos != nullptr ? a.eos[r] : -1;
  int s = a.state[r];
  bool retire = false;
  for (long long i = done > 0 ? done : 0; i < (long long)m && i < (long long)a.out_stride; ++i) {
    if (s < 0 || s >= a.n_states) break;  // rule 1, for this token and every one behind it
    const long long t = a.out[(size_t)r * (size_t)a.out_stride + (size_t)i];
    const int lo = fsm_clamp(a.offsets[s], a.n_edges);
    int hi = fsm_clamp(a.offsets[s + 1], a.n_edges);
    if (hi < lo) hi = lo;
    int to = -2;
    bool edge = false;
    if (t >= 0 && t <= 0x7fffffffll) {
      const int e = fsm_lower_bound(a.tokens, lo, hi, (int)t, lane);
      if (e < hi && a.tokens[e] == (int)t) {
        edge = true;
        to = a.next[e];
      }
    }
    if (edge) {
      if (to < 0 || to >= a.n_states) {
        s = -2;
        retire = true;
      } else {
        s = to;
        const int l2 = fsm_clamp(a.offsets[to], a.n_edges), h2 = fsm_clamp(a.offsets[to + 1], a.n_edges);
        if (h2 <= l2) retire = true;  // terminal
      }
    } else if (a.accept[s] != 0 && eos >= 0 && t == (long long)eos) {
      // the row's eos in an accepting state: the sampler has retired the row
    } else {
      s = -2;
      retire = true;
    }
  }
  if (lane == 0) {
    a.state[r] = s;
    a.n_fsm[r] = m;
    if (retire) {
      a.ids[r] = 0;
      a.pos[r] = -1;
      a.slots[r] = -1;
      a.remaining[r] = 0;
    }
  }
}

#endif  // QQQ_AMD_QQQ_GUIDED_HIP_H_
