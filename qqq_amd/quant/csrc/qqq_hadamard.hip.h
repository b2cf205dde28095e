// qqq_hadamard.hip.h -- the blocked Walsh-Hadamard transform of matrix rows (qqq_amd/quant/include/qqq_amd_rotate.h states the bits).
// Part of the single translation unit qqq_quant.hip (contraction off, correctly rounded divide, subnormals kept).
//
//   qqq_hadamard_kernel<T, VEC, LOG_TILE>   The matrix is a list of RUNS of 8 consecutive columns (of n columns when n < 8), numbered row
//       by row.  A thread owns one run in eight f64 registers from the load to the store; a workgroup of 2^(LOG_TILE-3) threads owns the
//       TILE of 2^LOG_TILE consecutive elements of that list.  n divides the tile and cols, so a tile holds whole blocks: 2048 / n of
//       them at n <= 2048 (LOG_TILE 11, 256 threads; the blocks may lie in different rows), one at n = 4096 (512 threads) and n = 8192
//       (1024 threads, 72 KB of LDS).  Small blocks therefore share a workgroup and every load and store is one run of 16 (fp16) or
//       2 x 16 (f32) bytes per thread where the pointers and strides allow it (VEC), element by element otherwise.
//       The stages h = 1, 2, 4 run in the registers.  Every further group of three stages is one trip through LDS: the tile goes out in
//       the layout the thread holds, comes back with the three index bits of the next stages in the register index, and the same
//       register butterflies run again; a last trip brings the runs back.  Moving values changes no bit, and each output of a stage is
//       the one add the header states, of the outputs of the stage before: the stage ORDER per value is the header's.  The tile's LDS
//       image is padded by one double per eight (index + index / 8): a thread's eight-element run and a stage group's strided octet
//       both spread over the banks.  Nothing passes between workgroups; a thread past the last run computes zeros and stores nothing.
//       The kernel is bound by f64 vector instructions, not by memory or LDS (measured: fewer trips with 16-element runs bought
//       nothing), so the two per-element extras are kept short: a sign is a flip of the sign bit, and the divide is had_div below.
#ifndef QQQ_AMD_QQQ_HADAMARD_HIP_H_
#define QQQ_AMD_QQQ_HADAMARD_HIP_H_

#include <cstdint>

#pragma clang fp contract(off)

static constexpr int HAD_RUN = 8;          // elements a thread owns
static constexpr int HAD_MAX_N = 8192;

struct qqq_hadamard_args {
  const void* X;
  void* Y;
  const signed char* sign;  // NULL: all +1
  long long ldx, ldy;
  long long units;          // runs in the matrix: rows * units_per_row
  int units_per_row;        // cols / run
  int run;                  // min(n, 8)
  int n, log2n;
  double d;                 // (double)sqrtf((float)n)
  double rd;                // 1 / d, correctly rounded (the host's divide)
};

typedef unsigned int had_u2 __attribute__((ext_vector_type(2)));
typedef unsigned int had_u4 __attribute__((ext_vector_type(4)));
typedef float had_f4 __attribute__((ext_vector_type(4)));

template <bool VEC>
__device__ __forceinline__ void had_load(const _Float16* p, const int run, double (&v)[HAD_RUN]) {
  if (VEC) {
    union {
      had_u4 q;
      _Float16 h[HAD_RUN];
    } u;
    u.q = *reinterpret_cast<const had_u4*>(p);
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) v[j] = static_cast<double>(static_cast<float>(u.h[j]));
  } else {
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) v[j] = j < run ? static_cast<double>(static_cast<float>(p[j])) : 0.0;
  }
}

template <bool VEC>
__device__ __forceinline__ void had_load(const float* p, const int run, double (&v)[HAD_RUN]) {
  if (VEC) {
    const had_f4 a = *reinterpret_cast<const had_f4*>(p), b = *reinterpret_cast<const had_f4*>(p + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) v[j] = j < run ? static_cast<double>(p[j]) : 0.0;
  }
}

// f64 -> f32 -> fp16: the double rounding is the contract
template <bool VEC>
__device__ __forceinline__ void had_store(_Float16* p, const int run, const float (&y)[HAD_RUN]) {
  if (VEC) {
    union {
      had_u4 q;
      _Float16 h[HAD_RUN];
    } u;
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) u.h[j] = static_cast<_Float16>(y[j]);
    *reinterpret_cast<had_u4*>(p) = u.q;
  } else {
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j)
      if (j < run) p[j] = static_cast<_Float16>(y[j]);
  }
}

template <bool VEC>
__device__ __forceinline__ void had_store(float* p, const int run, const float (&y)[HAD_RUN]) {
  if (VEC) {
    had_f4 a, b;
    a.x = y[0], a.y = y[1], a.z = y[2], a.w = y[3], b.x = y[4], b.y = y[5], b.z = y[6], b.w = y[7];
    *reinterpret_cast<had_f4*>(p) = a;
    *reinterpret_cast<had_f4*>(p + 4) = b;
  } else {
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j)
      if (j < run) p[j] = y[j];
  }
}

// x * sign for sign = +-1: the sign bit flipped where the entry is negative (the same bits as the product, zeros included)
__device__ __forceinline__ double had_signed(const double x, const unsigned negative) {
  return __longlong_as_double(__double_as_longlong(x) ^ (static_cast<long long>(negative & 1u) << 63));
}

// v / d correctly rounded, for THIS d, in three instructions instead of the division sequence.  q = RN(v * rd) is within 1.5 ulp of
// v / d; r = v - q d is exact in one fma (d = sqrtf(n) has 24 significant bits: r is a multiple of ulp(q) * ulp24(d) below 2^26 of
// them); RN(q + r * rd) is then off the true quotient by at most 1.5 ulp * 2^-53, while a quotient by a 24-bit divisor that is no
// double itself lies at least 2^-25 ulp from every rounding boundary: the fma rounds as the exact quotient does.  r == 0 (the product
// was exact: every power-of-four n, and v = +-0) keeps q and its sign; inf and NaN (r is NaN) keep q as well.
__device__ __forceinline__ double had_div(const double v, const double d, const double rd) {
  const double q = v * rd;
  const double r = __builtin_fma(-q, d, v);
  return __builtin_fabs(r) > 0.0 ? __builtin_fma(r, rd, q) : q;
}

// the stage of register-index bit K: (v[i], v[i + 2^K]) <- (v[i] + v[i + 2^K], v[i] - v[i + 2^K]) for every i with that bit clear
template <int K>
__device__ __forceinline__ void had_stage(double (&v)[HAD_RUN]) {
#pragma unroll
  for (int i = 0; i < HAD_RUN; ++i)
    if ((i & (1 << K)) == 0) {
      const double a = v[i], b = v[i + (1 << K)];
      v[i] = a + b;
      v[i + (1 << K)] = a - b;
    }
}

// the padded LDS index of register j of thread t when the register index holds the tile-index bits base ... base + 2
__device__ __forceinline__ int had_slot(const int t, const int j, const int base) {
  const int idx = (t & ((1 << base) - 1)) | (j << base) | ((t >> base) << (base + 3));
  return idx + (idx >> 3);
}

template <typename T, bool VEC, int LOG_TILE>
__global__ __launch_bounds__(1 << (LOG_TILE - 3)) void qqq_hadamard_kernel(const qqq_hadamard_args a) {
  constexpr int NT = 1 << (LOG_TILE - 3);
  __shared__ double tile[NT * (HAD_RUN + 1)];
  const int t = threadIdx.x;
  const long long u = static_cast<long long>(blockIdx.x) * NT + t;
  const bool live = u < a.units;
  double v[HAD_RUN];
  T* yp = nullptr;
  if (live) {
    const long long row = u / a.units_per_row;
    const int col = static_cast<int>(u - row * a.units_per_row) * a.run;
    had_load<VEC>(static_cast<const T*>(a.X) + row * a.ldx + col, a.run, v);
    yp = static_cast<T*>(a.Y) + row * a.ldy + col;
    if (a.sign) {
      const signed char* s = a.sign + (col & (a.n - 1));
      if (VEC) {  // the run's eight entries in one load (the host takes VEC only with an 8-byte aligned sign)
        const had_u2 w = *reinterpret_cast<const had_u2*>(s);
#pragma unroll
        for (int j = 0; j < HAD_RUN; ++j) v[j] = had_signed(v[j], (j < 4 ? w.x : w.y) >> (8 * (j & 3) + 7));
      } else {
#pragma unroll
        for (int j = 0; j < HAD_RUN; ++j)
          if (j < a.run) v[j] = had_signed(v[j], s[j] < 0);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) v[j] = 0.0;
  }
  // h = 1, 2, 4 (those below n)
  had_stage<0>(v);
  if (a.log2n > 1) had_stage<1>(v);
  if (a.log2n > 2) had_stage<2>(v);
  int base = 0;  // the tile-index bits the register index holds now
  for (int done = 3; done < a.log2n; done += 3) {
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) tile[had_slot(t, j, base)] = v[j];
    __syncthreads();
    base = done < LOG_TILE - 3 ? done : LOG_TILE - 3;  // the last trip of a tile whose bits are no multiple of three overlaps the one before
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) v[j] = tile[had_slot(t, j, base)];
    __syncthreads();
    if (base + 0 >= done && base + 0 < a.log2n) had_stage<0>(v);
    if (base + 1 >= done && base + 1 < a.log2n) had_stage<1>(v);
    if (base + 2 >= done && base + 2 < a.log2n) had_stage<2>(v);
  }
  if (base != 0) {
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) tile[had_slot(t, j, base)] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) v[j] = tile[had_slot(t, j, 0)];
  }
  if (live) {
    float y[HAD_RUN];
#pragma unroll
    for (int j = 0; j < HAD_RUN; ++j) y[j] = static_cast<float>(had_div(v[j], a.d, a.rd));
    had_store<VEC>(yp, a.run, y);
  }
}

#endif  // QQQ_AMD_QQQ_HADAMARD_HIP_H_
