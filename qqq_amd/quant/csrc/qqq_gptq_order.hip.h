// qqq_gptq_order.hip.h -- the two device ops of GPTQ with act-order and static groups (qqq_amd/quant/include/qqq_amd_gptq_order.h).  Part
// of the single translation unit qqq_quant.hip (contraction off), behind qqq_gptq.hip.h, whose bodies both kernels run:
//
//   qqq_gptq_group_scales_kernel   every (row, group) pair's grouped scale in one launch.  A wave takes a pair and runs
//       gptq_scales_body<64> on the group's 128 values: lane t takes the columns t and t + 64, the same xor butterflies reduce -- the walk of
//       qqq_gptq_scales_kernel<64> over a 128-column slice, so the bits are that kernel's by construction.  Four pairs per workgroup.
//   qqq_gptq_block_cols_kernel<COUNT>   gptq_block_body in grouped arithmetic with a scale per (row, column).  After the permutation of
//       act-order a block holds columns of many groups: while it loads its weights a lane reads the group index of each of its COUNT / 8
//       columns (clamped into [0, groups)) and gathers scales[row, gidx[col]] into registers, COUNT / 8 more VGPRs.  In step I the
//       owner's scale travels with the owner's weight by a second eight-lane move, so every lane still computes q and e on the same
//       bits.  No LDS beyond the block of Hinv.
#ifndef QQQ_AMD_QQQ_GPTQ_ORDER_HIP_H_
#define QQQ_AMD_QQQ_GPTQ_ORDER_HIP_H_

#include "qqq_gptq.hip.h"

#pragma clang fp contract(off)

struct qqq_gptq_group_scales_args {
  const float* W;
  float* out;
  long long ldw, lds, pairs;
  int groups, mse;
};

__global__ __launch_bounds__(GPTQ_SC_NT) void qqq_gptq_group_scales_kernel(const qqq_gptq_group_scales_args a) {
  const long long pair_raw = (long long)blockIdx.x * (GPTQ_SC_NT / 64) + threadIdx.x / 64;
  const bool live = pair_raw < a.pairs;
  const long long pair = live ? pair_raw : a.pairs - 1;
  const long long row = pair / a.groups, g = pair % a.groups;
  gptq_scales_body<64>(a.W + row * a.ldw + g * 128, 128, true, a.mse != 0, live, a.out + row * a.lds + g);
}

struct qqq_gptq_block_cols_args {
  const float* W1;
  const float* Hinv1;
  const float* scales;
  const int* gidx;
  float* Q1;
  float* Err1;
  long long ldw, ldh, lds, ldq, lde;
  int rows, groups;
};

// the scale source of gptq_sweep with one scale per (row, column): the lane's columns' scales in registers, the owner's moved in step I
template <int COUNT>
struct gptq_col_scales {
  float s[COUNT / 8];
  __device__ __forceinline__ gptq_col_scales(const qqq_gptq_block_cols_args& a, const long long row, const int l) {
    const float* sp = a.scales + row * a.lds;
    const int* gp = a.gidx + 4 * l;
#pragma unroll
    for (int c = 0; c < COUNT / 32; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) s[4 * c + e] = sp[min(max(gp[32 * c + e], 0), a.groups - 1)];
  }
  template <int COUNT_, int I>
  __device__ __forceinline__ float step() const {
    static_assert(COUNT_ == COUNT, "the scales are those of this block");
    return __shfl(s[4 * (I / 32) + I % 4], (I % 32) / 4, GPTQ_LANES);
  }
};

template <int COUNT>
__global__ __launch_bounds__(GPTQ_NT) void qqq_gptq_block_cols_kernel(const qqq_gptq_block_cols_args a) {
  gptq_block_body<COUNT, true, gptq_col_scales<COUNT>>(a);
}

#endif  // QQQ_AMD_QQQ_GPTQ_ORDER_HIP_H_
