// qqq_step.hip.h -- the decode loop's sample-and-advance step (include/qqq_amd_step.h): the fused token sampler's row (qqq_sample_row of
// qqq_sample.hip.h, the same code qqq_sample_tokens runs) with an epilogue that advances the row's decode state in device memory.  Part of
// the single translation unit qqq_w4a8.hip.
//
//   qqq_step_advance_kernel   One workgroup per row.  Every lane reads the row's variate u[r, tick[r] % u_stride] in front of the sampler's
//                             first barrier (qqq_step_emit::variate); the one lane that ends up with the token runs qqq_step_emit behind it -- the only writer of the
//                             row's state, with ordinary vector stores.  Every index is checked against its array before it is used.
#ifndef QQQ_AMD_QQQ_STEP_HIP_H_
#define QQQ_AMD_QQQ_STEP_HIP_H_

struct qqq_step_emit {
  const float* uu;
  int* tick;
  long long* ids;
  long long* pos;
  long long* slots;
  const int* block_table;
  int* remaining;
  const int* eos;
  long long* out;
  int* n_out;
  int u_stride, table_stride, out_stride, block_shift;

  __device__ __forceinline__ float variate(const int r) const {
    return uu[(size_t)r * u_stride + (unsigned)tick[r] % (unsigned)u_stride];
  }

  __device__ __forceinline__ void operator()(const int r, const long long tok) const {
    tick[r] = (int)((unsigned)tick[r] + 1u);
    int rem = remaining[r];
    if (rem <= 0) return;  // an idle row
    const int n = n_out[r];
    const bool room = n >= 0 && n < out_stride;
    if (room) {
      out[(size_t)r * out_stride + n] = tok;
      n_out[r] = n + 1;
    }
    rem -= 1;
    const long long p = pos[r] + 1;
    const long long blk = p >> block_shift;
    if (tok == (long long)eos[r] || !room || n + 1 >= out_stride || p < 0 || blk >= (long long)table_stride) rem = 0;
    if (rem > 0) {
      const long long bs = 1ll << block_shift;
      ids[r] = tok;
      pos[r] = p;
      slots[r] = (long long)block_table[(size_t)r * table_stride + blk] * bs + (p & (bs - 1));
      remaining[r] = rem;
    } else {
      ids[r] = 0;
      pos[r] = -1;
      slots[r] = -1;
      remaining[r] = 0;
    }
  }
};

__global__ __launch_bounds__(SMP_NT) void qqq_step_advance_kernel(const unsigned short* __restrict__ logits, const int ld,
                                                                  const float* __restrict__ temperature, const int* __restrict__ top_k,
                                                                  const float* __restrict__ top_p, const qqq_step_emit st,
                                                                  const int vocab) {
  qqq_sample_row(logits, ld, temperature, top_k, top_p, vocab, blockIdx.x, st);
}

#endif  // QQQ_AMD_QQQ_STEP_HIP_H_
