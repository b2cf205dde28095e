// qqq_fakequant.hip.h -- the symmetric fake-quantisation of the rows of a column-scaled fp16 matrix, the inner step of the smoothing
// search (qqq_amd/quant/include_ops/qqq_amd_fakequant.h states the bits).  Part of the single translation unit qqq_quant.hip
// (contraction off, correctly rounded divide, subnormals kept).
//
//   The matrix is a list of UNITS of 8 consecutive columns: one 16-byte load, one 16-byte store, and one 16-byte load of the eight
//   column scales per unit.  A unit's scaled values t = fp16(x op c) are kept as fp16 bits in four registers.
//
//   qqq_fake_quant_row_kernel<UPT>    one scale per row.  A workgroup of 256 threads owns one row; thread i owns the units i, i + 256, ...
//       UPT > 0: the row has at most 256 * UPT units (cols <= 2048 * UPT, UPT = 1, 2, 4, 8) and is read ONCE: every thread keeps its UPT
//       units of t in registers across the reduction.  UPT == 0: any width; the row is read, reduced, and read again (t is computed
//       twice from the same operands: the same bits).  In place is safe in both: a thread writes only units it alone reads, after it
//       read them, and every first-pass read is over before the barrier of the reduction.
//       The reduction of (min, max) goes through the wave (xor shuffles) and then four LDS slots per value.  min and max of fp16
//       values are exact in f32, in any order.
//   qqq_fake_quant_group_kernel       one scale per (row, 128 columns).  A thread owns ONE unit of the flat list rows * cols / 8; the 16
//       units of a group are 16 consecutive, 16-aligned lanes (cols % 128 == 0), so the reduction is four xor shuffles of width 16 and
//       never leaves them.  Lanes past the last unit hold zeros and store nothing (whole groups of 16 at a time).
//
//   Nothing passes between workgroups.  Every index into a matrix is 64-bit.
#ifndef QQQ_AMD_QQQ_FAKEQUANT_HIP_H_
#define QQQ_AMD_QQQ_FAKEQUANT_HIP_H_

#include <cstdint>

#pragma clang fp contract(off)

static constexpr int FQ_NT = 256;    // threads of a workgroup
static constexpr int FQ_UNIT = 8;    // columns of a unit: 16 bytes of fp16
static constexpr int FQ_MAX_UPT = 8; // units a thread keeps in registers: rows of up to 16384 columns are read once

struct qqq_fake_quant_args {
  const _Float16* X;
  _Float16* Y;
  const _Float16* c;  // NULL: t = x
  long long ldx, ldy;
  long long units;    // rows * units_per_row
  int units_per_row;  // cols / 8
  int divide;         // 1: t = x / c, 0: t = x * c
  float qmax;         // 127 or 7
};

typedef unsigned int fq_u4 __attribute__((ext_vector_type(4)));

union fq_unit {
  fq_u4 q;
  _Float16 h[FQ_UNIT];
};

// t = fp16(f32(x) op f32(c)) for the eight columns of unit `u` of a row, and the running (min, max) of t
__device__ __forceinline__ fq_unit fq_scaled(const _Float16* xrow, const _Float16* c, const int u, const int divide, float& mn, float& mx) {
  fq_unit x;
  x.q = *reinterpret_cast<const fq_u4*>(xrow + static_cast<long long>(u) * FQ_UNIT);
  if (c != nullptr) {
    fq_unit s;
    s.q = *reinterpret_cast<const fq_u4*>(c + static_cast<long long>(u) * FQ_UNIT);
#pragma unroll
    for (int j = 0; j < FQ_UNIT; ++j) {
      const float a = static_cast<float>(x.h[j]), b = static_cast<float>(s.h[j]);
      x.h[j] = static_cast<_Float16>(divide ? a / b : a * b);
    }
  }
#pragma unroll
  for (int j = 0; j < FQ_UNIT; ++j) {
    const float v = static_cast<float>(x.h[j]);
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  return x;
}

// the scale of a row or group from its min(min t, 0) and max(max t, 0): max(fp16(a / qmax), 2^-23), as f32
__device__ __forceinline__ float fq_scale(const float mn, const float mx, const float qmax) {
  const float a = fmaxf(-mn, mx);
  const float s = static_cast<float>(static_cast<_Float16>(a / qmax));
  return fmaxf(s, 1.1920928955078125e-07f);
}

__device__ __forceinline__ void fq_store(_Float16* yrow, const int u, fq_unit t, const float s, const float qmax) {
#pragma unroll
  for (int j = 0; j < FQ_UNIT; ++j) {
    const float q = static_cast<float>(static_cast<_Float16>(static_cast<float>(t.h[j]) / s));
    float r = rintf(q);  // half to even
    r = fminf(fmaxf(r, -qmax), qmax) + 0.0f;  // -0 + 0 = +0: the reference's integer zero point
    t.h[j] = static_cast<_Float16>(r * s);
  }
  *reinterpret_cast<fq_u4*>(yrow + static_cast<long long>(u) * FQ_UNIT) = t.q;
}

template <int UPT>
__global__ __launch_bounds__(FQ_NT) void qqq_fake_quant_row_kernel(const qqq_fake_quant_args a) {
  __shared__ float red[2][FQ_NT / 64];
  const int tid = threadIdx.x;
  const long long row = blockIdx.x;
  const _Float16* xrow = a.X + row * a.ldx;
  _Float16* yrow = a.Y + row * a.ldy;
  const int units = a.units_per_row;
  float mn = 0.f, mx = 0.f;  // the zero the reference clamps both against
  fq_unit t[UPT > 0 ? UPT : 1];
  if (UPT > 0) {
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
      const int u = tid + k * FQ_NT;
      if (u < units) t[k] = fq_scaled(xrow, a.c, u, a.divide, mn, mx);
    }
  } else {
    for (int u = tid; u < units; u += FQ_NT) (void)fq_scaled(xrow, a.c, u, a.divide, mn, mx);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, m, 64));
    mx = fmaxf(mx, __shfl_xor(mx, m, 64));
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = mn;
    red[1][tid >> 6] = mx;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < FQ_NT / 64; ++w) {
    mn = fminf(mn, red[0][w]);
    mx = fmaxf(mx, red[1][w]);
  }
  const float s = fq_scale(mn, mx, a.qmax);
  if (UPT > 0) {
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
      const int u = tid + k * FQ_NT;
      if (u < units) fq_store(yrow, u, t[k], s, a.qmax);
    }
  } else {
    float m0 = 0.f, m1 = 0.f;
    for (int u = tid; u < units; u += FQ_NT) fq_store(yrow, u, fq_scaled(xrow, a.c, u, a.divide, m0, m1), s, a.qmax);
  }
}

__global__ __launch_bounds__(FQ_NT) void qqq_fake_quant_group_kernel(const qqq_fake_quant_args a) {
  const long long unit = static_cast<long long>(blockIdx.x) * FQ_NT + threadIdx.x;
  const bool live = unit < a.units;
  const long long row = live ? unit / a.units_per_row : 0;
  const int u = live ? static_cast<int>(unit - row * a.units_per_row) : 0;
  float mn = 0.f, mx = 0.f;
  fq_unit t;
  t.q = fq_u4{0u, 0u, 0u, 0u};
  if (live) t = fq_scaled(a.X + row * a.ldx, a.c, u, a.divide, mn, mx);
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, m, 16));
    mx = fmaxf(mx, __shfl_xor(mx, m, 16));
  }
  if (live) fq_store(a.Y + row * a.ldy, u, t, fq_scale(mn, mx, a.qmax), a.qmax);
}

#endif  // QQQ_AMD_QQQ_FAKEQUANT_HIP_H_
