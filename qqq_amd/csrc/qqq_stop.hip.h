// qqq_stop.hip.h -- stop sequences, stop token ids and the minimum length of a completion (include/qqq_amd_stop.h): two integer
// kernels around a decode loop's sampler, both inside its captured step.  Part of the single translation unit qqq_w4a8.hip.
//
//   qqq_ban_tokens_kernel   One wave per logits row (4 per workgroup).  A row whose completion index is below the row's minimum length
//                           gets fp16 -inf at its eos (lane 32) and at ban_ids[lane] (lanes 0 ... n_ban - 1): at most 33 two-byte stores,
//                           every one to a column checked against [0, vocab); duplicates store the same bits twice.
//   qqq_stop_check_kernel   One wave per row (4 per workgroup).  Lanes 0 ... 31 hold one stop sequence each, lanes 32 ... 63 one end id
//                           each; the new ends of the completion are walked in ascending order and every lane tests its entry at the end
//                           (a sequence only from the row's minimum length on), the row's eos is tested by the whole wave, a ballot finds
//                           the winner (eos, then the end ids, then the lowest sequence), and the walk stops at the first match.
//                           The wave reads n_seen[r] at its start and lane 0 writes it at its end; lanes 0 ... G - 1 retire the row's
//                           ids / pos / slots.  Every token index is checked against its array before it is used, every table index
//                           against stop_stride.  One body serves 4-byte and 8-byte tokens.
#ifndef QQQ_AMD_QQQ_STOP_HIP_H_
#define QQQ_AMD_QQQ_STOP_HIP_H_

static constexpr int STOP_NT = 256;
static constexpr int STOP_WAVES = STOP_NT / 64;
static constexpr int STOP_MAX = 32;        // stop sequences, their length, stop token ids
static constexpr int STOP_MAX_GROUP = 16;

__global__ __launch_bounds__(STOP_NT) void qqq_ban_tokens_kernel(unsigned short* __restrict__ logits, const int ld,
                                                                 const int* __restrict__ n_out, const int base,
                                                                 const int* __restrict__ min_new, const int* __restrict__ eos,
                                                                 const int* __restrict__ ban_ids, const int n_ban, const int group,
                                                                 const int total, const int vocab) {
  const int row = blockIdx.x * STOP_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= total) return;
  const int r = row / group, j = row - r * group;
  const long long index = (long long)n_out[r] + (long long)base + (long long)j;
  if (index >= (long long)min_new[r]) return;
  int t = -1;
  if (lane < n_ban)  // n_ban <= 32
    t = ban_ids[lane];
  else if (lane == STOP_MAX)
    t = eos[r];
  if (t >= 0 && t < vocab) logits[(size_t)row * ld + t] = (unsigned short)0xFC00u;
}

struct qqq_stop_state {
  const void* tokens;
  const int* base;
  const int* first;  // may be NULL
  const int* n_out;
  const int* stop_ids;
  const int* stop_len;
  const int* end_ids;
  const int* eos;  // may be NULL
  const int* min_new;
  int* n_seen;
  int* n_trim;
  int* stop_hit;
  long long* ids;
  long long* pos;
  long long* slots;
  long long* start;  // may be NULL
  int* remaining;
  int token_bytes, tok_stride, stop_stride, n_stop, n_end, group, rows;

  // c_r[i] -> v; false: the index holds no token
  __device__ __forceinline__ bool token(const int r, const int b, const long long i, long long& v) const {
    const long long at = (long long)b + i;
    if (at < 0) {
      if (first == nullptr) return false;
      v = (long long)first[r];
      return true;
    }
    if (at >= (long long)tok_stride) return false;
    const size_t idx = (size_t)r * (size_t)tok_stride + (size_t)at;
    v = token_bytes == 8 ? static_cast<const long long*>(tokens)[idx] : (long long)static_cast<const int*>(tokens)[idx];
    return true;
  }
};

__global__ __launch_bounds__(STOP_NT) void qqq_stop_check_kernel(const qqq_stop_state st) {
  const int r = blockIdx.x * STOP_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= st.rows) return;
  const long long m = (long long)st.n_out[r] + 1;
  const int seen = st.n_seen[r];
  const long long a = seen > 0 ? (long long)seen : 0ll;
  if (a >= m) return;  // wave-uniform: nothing new to check, nothing written
  const int b = st.base[r];
  const long long lowest = (long long)st.min_new[r];
  const int eos = st.eos != nullptr ? st.eos[r] : -1;

  // this lane's entry: a stop sequence (lanes 0 ... 31) or an end id (lanes 32 ... 63)
  const bool is_end = lane >= STOP_MAX;
  const int s = lane & (STOP_MAX - 1);
  int len = 0, end_id = -1;
  if (!is_end) {
    if (s < st.n_stop) {
      len = st.stop_len[s];
      if (len < 1 || len > st.stop_stride) len = 0;
    }
  } else if (s < st.n_end) {
    end_id = st.end_ids[s];
  }

  long long trim = -1;
  int hit = -1;
  for (long long e = a + 1; e <= m; ++e) {
    bool match = false;
    long long v;
    const bool last = st.token(r, b, e - 1, v);  // wave-uniform
    if (last && eos >= 0 && v == (long long)eos) {  // the row's eos: before every table entry, at any length
      hit = st.n_stop + st.n_end;
      trim = m - e;
      break;
    }
    if (is_end) {
      match = end_id >= 0 && last && v == (long long)end_id;
    } else if (len >= 1 && (long long)len <= e && e >= lowest) {
      const int* seq = st.stop_ids + (size_t)s * (size_t)st.stop_stride;  // len >= 1: s < n_stop, stop_ids is not NULL
      match = true;
      for (int k = 0; k < len && match; ++k) match = st.token(r, b, e - len + k, v) && v == (long long)seq[k];
    }
    const unsigned long long mask = __ballot(match);
    if (mask != 0ull) {  // wave-uniform
      const unsigned ends = (unsigned)(mask >> 32), seqs = (unsigned)(mask & 0xffffffffull);
      if (ends != 0u) {
        hit = st.n_stop + __builtin_ctz(ends);
        trim = m - e;
      } else {
        hit = __builtin_ctz(seqs);
        trim = m - e + (long long)__shfl(len, hit);
      }
      break;
    }
  }

  if (hit >= 0) {
    if (lane < st.group) {
      const size_t at = (size_t)r * (size_t)st.group + (size_t)lane;
      st.ids[at] = 0;
      st.pos[at] = -1;
      st.slots[at] = -1;
    }
    if (lane == 0) {
      st.n_trim[r] = (int)trim;
      st.stop_hit[r] = hit;
      if (st.start != nullptr) st.start[r] = -1;
      st.remaining[r] = 0;
    }
  }
  if (lane == 0) st.n_seen[r] = (int)m;
}

#endif  // QQQ_AMD_QQQ_STOP_HIP_H_
