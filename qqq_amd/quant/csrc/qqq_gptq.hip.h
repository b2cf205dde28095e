// qqq_gptq.hip.h -- the two device ops of the GPTQ quantiser (qqq_amd/quant/include/qqq_amd_quant.h).  Part of the single translation
// unit qqq_quant.hip, which is built with floating-point contraction off: the arithmetic below is the statement of the result's bits.
//
//   qqq_gptq_block_kernel<COUNT, GROUPED>   the column sweep of one block, one launch.  A workgroup of 128 threads owns 16 rows and a copy of the
//       COUNT x COUNT block of Hinv in LDS (64 KB at COUNT = 128: two workgroups per CU).  Eight lanes share a row: lane l keeps the
//       columns 32 c + 4 l ... + 3 of every 32-column chunk c in registers, so the live work of a step stays spread over the eight lanes
//       until the last chunk, and a lane's share of a row of Hinv is one 16-byte LDS read per chunk (the sixteen rows of the workgroup
//       read the same eight addresses: a broadcast, no bank conflict).  The sweep is unrolled in full, so every register index is
//       static.  Step i: the owner's weight goes to the row's eight lanes by a cross-lane move, EVERY lane computes q and e from it (the
//       same arithmetic on the same bits: no divergence, no second move), the owner keeps them, and every lane updates its columns of
//       the chunks from i / 32 on.  The columns left of i in the chunk of i are updated too -- they are consumed already and never read
//       again.  Q1 and Err1 leave the registers once, behind the sweep.  No atomics, nothing between workgroups; a row beyond `rows`
//       computes a copy of the last row and stores nothing, so a row's bits do not know `rows` or the row's place.
//   qqq_gptq_scales_kernel<TPR>    the scale of a row from TPR threads (64 up to 512 columns -- four rows per workgroup -- else 256): the
//       row's max |w|, then with mse the 80 candidates' error sums in 80 registers per thread over one pass of the row, reduced through
//       the wave and, for TPR = 256, in wave order through LDS; one thread picks the earliest least.
// Both kernels are thin wrappers of a body (gptq_block_body, gptq_scales_body) that the kernels of qqq_gptq_order.hip.h run too: the sweep
// with a scale per (row, column) and the scales of every (row, group) pair share these bits by running this code.
#ifndef QQQ_AMD_QQQ_GPTQ_HIP_H_
#define QQQ_AMD_QQQ_GPTQ_HIP_H_

#include <utility>

#pragma clang fp contract(off)

static constexpr int GPTQ_NT = 128;          // threads of a sweep workgroup
static constexpr int GPTQ_LANES = 8;         // lanes that share a row
static constexpr int GPTQ_ROWS = GPTQ_NT / GPTQ_LANES;
static constexpr int GPTQ_SC_NT = 256;       // threads of a scales workgroup
static constexpr int GPTQ_GRID = 80;         // candidates of the shrink search: 1 - i / 100, i = 0 ... 79
static constexpr int GPTQ_SC_NARROW = 512;   // up to this many columns a wave takes a row

typedef float gptq_f4 __attribute__((ext_vector_type(4)));

// s * clamp(rint(w / s), -7, 7)   |   s * (clamp(rint(w / s) + 8, 0, 15) - 8)
__device__ __forceinline__ float gptq_quantise(const float w, const float s, const bool grouped) {
  const float r = rintf(w / s);
  if (grouped) return s * (fminf(fmaxf(r + 8.f, 0.f), 15.f) - 8.f);
  return s * fminf(fmaxf(r, -7.f), 7.f);
}

__device__ __forceinline__ float gptq_scale_of(const float range, const bool grouped) {
  return grouped ? (range + range) / 15.f : range / 7.f;
}

struct qqq_gptq_block_args {
  const float* W1;
  const float* Hinv1;
  const float* scale;
  float* Q1;
  float* Err1;
  long long ldw, ldh, ldq, lde;
  int rows;
};

// step I of the sweep, as a template: the sweep's 64 or 128 steps are instantiated one by one (a fold over an index sequence), because a
// loop of this size passes the compiler's limit for a full unroll and every register index below has to be a constant
template <int COUNT, bool GROUPED, int I>
__device__ __forceinline__ void gptq_step(float (&w)[COUNT / 8], float (&qv)[COUNT / 8], float (&ev)[COUNT / 8], const float* h_s, const int l,
                                          const float s) {
  constexpr int CH = COUNT / 32, C0 = I / 32, OWNER = (I % 32) / 4, IDX = 4 * C0 + I % 4;
  const float v = __shfl(w[IDX], OWNER, GPTQ_LANES);
  const float d = h_s[I * COUNT + I];
  const float q = gptq_quantise(v, s, GROUPED);
  const float err = (v - q) / d;
  qv[IDX] = l == OWNER ? q : qv[IDX];
  ev[IDX] = l == OWNER ? err : ev[IDX];
#pragma unroll
  for (int c = C0; c < CH; ++c) {
    const gptq_f4 h = *reinterpret_cast<const gptq_f4*>(&h_s[I * COUNT + 32 * c + 4 * l]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float prod = err * h[e];
      w[4 * c + e] = w[4 * c + e] - prod;
    }
  }
}

// the scale of a step: one per row here; qqq_gptq_order.hip.h has the per-column source.  A source is built from the kernel's arguments for
// the row and lane, and step<COUNT, I>() gives every lane of the row the scale of step I.
struct gptq_row_scale {
  float s;
  template <class ARGS>
  __device__ __forceinline__ gptq_row_scale(const ARGS& a, const long long row, const int) : s(a.scale[row]) {}
  template <int COUNT, int I>
  __device__ __forceinline__ float step() const {
    return s;
  }
};

template <int COUNT, bool GROUPED, class SCALE, int... I>
__device__ __forceinline__ void gptq_sweep(std::integer_sequence<int, I...>, float (&w)[COUNT / 8], float (&qv)[COUNT / 8],
                                           float (&ev)[COUNT / 8], const float* h_s, const int l, const SCALE& sc) {
  (gptq_step<COUNT, GROUPED, I>(w, qv, ev, h_s, l, sc.template step<COUNT, I>()), ...);
}

// the body of a sweep kernel: ARGS has W1, Hinv1, Q1, Err1, their strides and rows, and whatever SCALE reads
template <int COUNT, bool GROUPED, class SCALE, class ARGS>
__device__ __forceinline__ void gptq_block_body(const ARGS& a) {
  constexpr int CH = COUNT / 32;  // 32-column chunks
  __shared__ __attribute__((aligned(16))) float h_s[COUNT * COUNT];
  const int tid = threadIdx.x, l = tid & (GPTQ_LANES - 1), g = tid / GPTQ_LANES;
  for (int idx = tid; idx < COUNT * COUNT; idx += GPTQ_NT) h_s[idx] = a.Hinv1[(long long)(idx / COUNT) * a.ldh + idx % COUNT];

  const long long row_raw = (long long)blockIdx.x * GPTQ_ROWS + g;
  const bool live = row_raw < a.rows;
  const long long row = live ? row_raw : a.rows - 1;
  const SCALE sc(a, row, l);
  float w[CH * 4], qv[CH * 4], ev[CH * 4];
  const float* wp = a.W1 + row * a.ldw + 4 * l;
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      w[4 * c + e] = wp[32 * c + e];
      qv[4 * c + e] = 0.f;
      ev[4 * c + e] = 0.f;
    }
  __syncthreads();

  gptq_sweep<COUNT, GROUPED>(std::make_integer_sequence<int, COUNT>{}, w, qv, ev, h_s, l, sc);

  if (!live) return;
  float* qp = a.Q1 + row * a.ldq + 4 * l;
  float* ep = a.Err1 + row * a.lde + 4 * l;
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qp[32 * c + e] = qv[4 * c + e];
      ep[32 * c + e] = ev[4 * c + e];
    }
}

template <int COUNT, bool GROUPED>
__global__ __launch_bounds__(GPTQ_NT) void qqq_gptq_block_kernel(const qqq_gptq_block_args a) {
  gptq_block_body<COUNT, GROUPED, gptq_row_scale>(a);
}

struct qqq_gptq_scales_args {
  const float* W;
  float* out;
  long long ldw;
  int rows, cols, grouped, mse;
};

__device__ __forceinline__ float gptq_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float gptq_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the scale of the `cols` values at x from TPR threads, written to *out where `live` (every thread of the workgroup comes here, with
// workgroup-uniform cols, grouped and mse; TPR = 64: the workgroup's four waves take a row each).  Shared by the kernel below and by
// qqq_gptq_group_scales_kernel (qqq_gptq_order.hip.h), whose bits are this body's at 128 columns.
template <int TPR>
__device__ __forceinline__ void gptq_scales_body(const float* x, const int cols, const bool grouped, const bool mse, const bool live,
                                                 float* out) {
  constexpr int WAVES = GPTQ_SC_NT / 64;
  constexpr int RPW = GPTQ_SC_NT / TPR;  // rows of a workgroup: 4 (a wave each) or 1
  __shared__ float max_s[WAVES];
  __shared__ float cand_s[RPW][GPTQ_GRID];
  __shared__ float part_s[WAVES][GPTQ_GRID];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rl = tid / TPR, t = tid % TPR;

  float m = 0.f;
  for (int c = t; c < cols; c += TPR) m = fmaxf(m, fabsf(x[c]));
  m = gptq_wave_max(m);
  if (TPR > 64) {
    if (lane == 0) max_s[wave] = m;
    __syncthreads();
    m = max_s[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) m = fmaxf(m, max_s[w]);
  }
  const float xmax = m == 0.f ? 1.f : m;
  if (!mse) {  // (uniform)
    if (t == 0 && live) *out = gptq_scale_of(xmax, grouped);
    return;
  }

  for (int i = t; i < GPTQ_GRID; i += TPR) cand_s[rl][i] = gptq_scale_of((float)(1.0 - (double)i / 100.0) * xmax, grouped);
  __syncthreads();
  float acc[GPTQ_GRID];
#pragma unroll
  for (int i = 0; i < GPTQ_GRID; ++i) acc[i] = 0.f;
  for (int c = t; c < cols; c += TPR) {
    const float w = x[c];
#pragma unroll
    for (int i = 0; i < GPTQ_GRID; ++i) {
      const float diff = fabsf(gptq_quantise(w, cand_s[rl][i], grouped) - w);
      acc[i] += exp2f(2.4f * log2f(diff));  // |diff| ^ 2.4; 0 -> exp2(-inf) = 0
    }
  }
#pragma unroll
  for (int i = 0; i < GPTQ_GRID; ++i) {
    const float v = gptq_wave_sum(acc[i]);
    if (lane == 0) part_s[wave][i] = v;
  }
  __syncthreads();
  if (t == 0 && live) {
    float best = __builtin_inff(), s = cand_s[rl][0];
    for (int i = 0; i < GPTQ_GRID; ++i) {
      float tot;
      if (TPR > 64) {
        tot = part_s[0][i];
        for (int w = 1; w < WAVES; ++w) tot += part_s[w][i];
      } else {
        tot = part_s[wave][i];
      }
      if (tot < best) {
        best = tot;
        s = cand_s[rl][i];
      }
    }
    *out = s;
  }
}

template <int TPR>
__global__ __launch_bounds__(GPTQ_SC_NT) void qqq_gptq_scales_kernel(const qqq_gptq_scales_args a) {
  const long long row_raw = (long long)blockIdx.x * (GPTQ_SC_NT / TPR) + threadIdx.x / TPR;
  const bool live = row_raw < a.rows;
  const long long row = live ? row_raw : (long long)a.rows - 1;
  gptq_scales_body<TPR>(a.W + row * a.ldw, a.cols, a.grouped != 0, a.mse != 0, live, a.out + row);
}

#endif  // QQQ_AMD_QQQ_GPTQ_HIP_H_
