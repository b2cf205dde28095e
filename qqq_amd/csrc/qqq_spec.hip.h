// qqq_spec.hip.h -- the speculative decode loop's verify-and-advance step (include/qqq_amd_spec.h): G = draft_len + 1 draws per row by the
// fused token sampler's row (qqq_sample_row of qqq_sample.hip.h, the same code qqq_sample_tokens runs), then the row rule and the n-gram
// drafter over the row's history.  Part of the single translation unit qqq_w4a8.hip.
//
//   qqq_spec_draw_kernel      One workgroup per logits row r * G + j.  Every lane reads the variate u[r, (tick[r] * G + j) % u_stride] in
//                             front of the sampler's first barrier; the lane that ends up with the token stores it into the workspace.
//   qqq_spec_advance_kernel   One workgroup (4 waves) per row.  Lane 0 applies the row rule to the G draws: appends to hist, counts,
//                             decides whether the row goes on.  Then every lane scans hist for the drafter: for each end position c it
//                             counts how many tokens backwards from c equal the tokens backwards from the end, so one scan serves every
//                             n at once ("the largest i whose n-gram equals the last n tokens" is the largest c that matches n deep);
//                             the maxima are reduced by shuffles and LDS.  Lane 0 writes the next step's ids / pos / slots / start.  It
//                             is the only writer of the row's state, with ordinary vector stores; every index is checked against its
//                             array before it is used.
#ifndef QQQ_AMD_QQQ_SPEC_HIP_H_
#define QQQ_AMD_QQQ_SPEC_HIP_H_

static constexpr int SPEC_NT = 256;
static constexpr int SPEC_MAX_DRAFT = 15;
static constexpr int SPEC_MAX_NGRAM = 4;

struct qqq_spec_draw {
  const float* uu;
  const int* tick;
  long long* tokens;
  int u_stride, group;

  __device__ __forceinline__ float variate(const int i) const {
    const int r = i / group, j = i - r * group;
    return uu[(size_t)r * u_stride + ((unsigned)tick[r] * (unsigned)group + (unsigned)j) % (unsigned)u_stride];
  }

  __device__ __forceinline__ void operator()(const int i, const long long tok) const { tokens[i] = tok; }
};

__global__ __launch_bounds__(SMP_NT) void qqq_spec_draw_kernel(const unsigned short* __restrict__ logits, const int ld,
                                                               const float* __restrict__ temperature, const int* __restrict__ top_k,
                                                               const float* __restrict__ top_p, const qqq_spec_draw dr, const int vocab) {
  qqq_sample_row(logits, ld, temperature, top_k, top_p, vocab, blockIdx.x, dr);
}

struct qqq_spec_state {
  const long long* tokens;  // the draws, [rows, G]
  int* tick;
  long long* ids;
  long long* pos;
  long long* slots;
  long long* start;
  const int* block_table;
  int* remaining;
  const int* eos;
  int* hist;
  int* hist_len;
  int* n_out;
  int* n_acc;
  int table_stride, hist_stride, block_shift, draft_len, ngram_max;
};

__global__ __launch_bounds__(SPEC_NT) void qqq_spec_advance_kernel(const qqq_spec_state st) {
  __shared__ int sh_len;         // hist_len after the appends; 0: the row does not go on, nothing is left to do
  __shared__ long long sh_pos;   // p': the position of the last emitted token
  __shared__ int sh_rem;
  __shared__ int sh_best[SPEC_NT / 64][SPEC_MAX_NGRAM];

  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const int K = st.draft_len, G = K + 1;
  int* hist = st.hist + (size_t)r * st.hist_stride;
  long long* ids = st.ids + (size_t)r * G;
  long long* pos = st.pos + (size_t)r * G;
  long long* slots = st.slots + (size_t)r * G;

  if (tid == 0) {
    st.tick[r] = (int)((unsigned)st.tick[r] + 1u);
    int rem = st.remaining[r];
    int go = 0;
    if (rem > 0) {  // an active row
      const long long p = pos[0];
      int L = st.hist_len[r];
      bool alive = p >= 0 && L >= 1 && L < st.hist_stride;
      if (alive) {
        const long long* tok = st.tokens + (size_t)r * G;
        const long long eos = (long long)st.eos[r];
        int emitted = 0, accepted = 0;
        for (int j = 0; j <= K; ++j) {
          if (L >= st.hist_stride) {
            alive = false;
            break;
          }
          const long long s = tok[j];
          hist[L] = (int)s;
          L += 1;
          emitted += 1;
          rem -= 1;
          if (s == eos || rem <= 0) {
            alive = false;
            break;
          }
          if (j == K || s != ids[j + 1]) break;
          accepted += 1;
        }
        st.hist_len[r] = L;
        st.n_out[r] += emitted;
        st.n_acc[r] += accepted;
        const long long p1 = p + emitted;
        if (L >= st.hist_stride || ((p1 + K) >> st.block_shift) >= (long long)st.table_stride) alive = false;
        if (alive) {
          go = L;
          sh_pos = p1;
          sh_rem = rem;
        }
      }
      if (!alive) {
        for (int j = 0; j <= K; ++j) {
          ids[j] = 0;
          pos[j] = -1;
          slots[j] = -1;
        }
        st.start[r] = -1;
        st.remaining[r] = 0;
      }
    }
    sh_len = go;
  }
  __syncthreads();  // lane 0's appends to hist are visible to the workgroup behind it
  const int L = sh_len;
  if (L == 0) return;  // uniform: an idle row, or one that retired

  // ---- the drafter's scan: best[n - 1] = the largest c <= L - 2 with hist[c - t] == hist[L - 1 - t] for t = 0 ... n - 1
  const int nmax = st.ngram_max;
  int tail[SPEC_MAX_NGRAM], best[SPEC_MAX_NGRAM];
#pragma unroll
  for (int t = 0; t < SPEC_MAX_NGRAM; ++t) {
    tail[t] = (t < nmax && L - 1 - t >= 0) ? hist[L - 1 - t] : 0;
    best[t] = -1;
  }
  for (int c = tid; c <= L - 2; c += SPEC_NT) {
    bool run = true;
#pragma unroll
    for (int t = 0; t < SPEC_MAX_NGRAM; ++t) {
      run = run && t < nmax && c - t >= 0 && hist[c - t] == tail[t];
      if (run) best[t] = c;  // c ascends per lane: the last one is the lane's largest
    }
  }
#pragma unroll
  for (int t = 0; t < SPEC_MAX_NGRAM; ++t) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const int y = __shfl_xor(best[t], o);
      best[t] = y > best[t] ? y : best[t];
    }
    if ((tid & 63) == 0) sh_best[tid >> 6][t] = best[t];
  }
  __syncthreads();
  if (tid != 0) return;

  int src = -1;  // i + n: where the continuation of the match begins
  for (int t = nmax - 1; t >= 0 && src < 0; --t) {
    int c = -1;
#pragma unroll
    for (int w = 0; w < SPEC_NT / 64; ++w) c = sh_best[w][t] > c ? sh_best[w][t] : c;
    if (c >= 0) src = c + 1;
  }
  const long long p1 = sh_pos;
  const long long bs = 1ll << st.block_shift;
  const int* table = st.block_table + (size_t)r * st.table_stride;
  const long long last = (long long)hist[L - 1];
  ids[0] = last;
  for (int j = 0; j < K; ++j) {  // src + j - L < j: an entry written earlier in this loop
    const int at = src + j;
    ids[1 + j] = src < 0 ? last : (at < L ? (long long)hist[at] : ids[1 + at - L]);
  }
  for (int j = 0; j <= K; ++j) {  // (p1 + K) / block_size < table_stride was checked before the row was let on
    const long long q = p1 + j;
    pos[j] = q;
    slots[j] = (long long)table[q >> st.block_shift] * bs + (q & (bs - 1));
  }
  st.start[r] = p1;
  st.remaining[r] = sh_rem;
}

#endif  // QQQ_AMD_QQQ_SPEC_HIP_H_
