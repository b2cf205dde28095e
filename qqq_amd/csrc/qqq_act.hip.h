// qqq_act.hip.h -- activation quantisers of a Llama decoder block: RMSNorm (+ residual add) and SiLU·mul, each fused with the per-token
// int8 quantisation the next QuantLinear needs (include/qqq_amd_act.h).  Part of the single translation unit qqq_w4a8.hip.
//
// Same shape as qqq_dynamic_quant_kernel: one workgroup per token row, the row held in registers (VPT 16-byte vectors per thread), NT = 1024
// for few rows or long rows.  The quantisation step (qqq_act_quant_row) is bit for bit the one of qqq_dynamic_quant_kernel:
//   s1 = float(fp16(amax * (1/127))),  q = rint(y / s1) (correctly rounded quotient), clamp [-128, 127], all-zero row -> 0 codes.
#ifndef QQQ_AMD_QQQ_ACT_HIP_H_
#define QQQ_AMD_QQQ_ACT_HIP_H_

// workgroup reductions over NT / 64 waves; `red` is NT / 64 floats of LDS that the caller does not reuse before the next barrier
template <int NT>
__device__ __forceinline__ float qqq_wg_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) v += red[w];
  return v;
}

template <int NT>
__device__ __forceinline__ float qqq_wg_max(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) v = fmaxf(v, red[w]);
  return v;
}

// Per-token int8 quantisation of a row held in registers (vector idx = threadIdx.x + i * NT, valid below nvec): the arithmetic of
// qqq_dynamic_quant_kernel (qqq_small.hip.h), which stays as it is -- see there for why the near-tie elements take the exact division.
template <int VPT, int NT>
__device__ __forceinline__ void qqq_act_quant_row(const h8 (&v)[VPT], const int nvec, int8_t* __restrict__ xq_row,
                                                  float* __restrict__ s1_row, float* red) {
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x;
  h2 amax2 = {(_Float16)0, (_Float16)0};
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    if (tid + i * NT < nvec) {
      const u4v bits = __builtin_bit_cast(u4v, v[i]);
      const h2 m0 = __builtin_elementwise_max(__builtin_bit_cast(h2, bits.x & 0x7fff7fffu), __builtin_bit_cast(h2, bits.y & 0x7fff7fffu));
      const h2 m1 = __builtin_elementwise_max(__builtin_bit_cast(h2, bits.z & 0x7fff7fffu), __builtin_bit_cast(h2, bits.w & 0x7fff7fffu));
      amax2 = __builtin_elementwise_max(amax2, __builtin_elementwise_max(m0, m1));
    }
  }
  const float amax = qqq_wg_max<NT>(fmaxf((float)amax2[0], (float)amax2[1]), red);
  const float scale = (float)(_Float16)__fmul_rn(amax, 1.0f / 127.0f);
  if (tid == 0) *s1_row = scale;
  const float rinv = (scale > 0.f) ? __frcp_rn(scale) : 0.f;
  int2* qr = reinterpret_cast<int2*>(xq_row);
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = tid + i * NT;
    if (idx < nvec) {
      float q[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xe = (float)v[i][e];
        const float p = xe * rinv;
        q[e] = rintf(p);
        const bool near_tie = fabsf(p - q[e]) > 0.4995f;
        if (__builtin_amdgcn_ballot_w64(near_tie) != 0) {
          const float qd = (scale > 0.f) ? rintf(__fdiv_rn(xe, scale)) : 0.f;
          q[e] = near_tie ? qd : q[e];
        }
      }
      unsigned lo = 0, hi = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned byte = (unsigned)((int)fminf(fmaxf(q[e], -128.f), 127.f)) & 0xFFu;
        if (e < 4)
          lo |= byte << (8 * e);
        else
          hi |= byte << (8 * (e - 4));
      }
      qr[idx] = make_int2((int)lo, (int)hi);
    }
  }
}

// LlamaRMSNorm (transformers, fp16 input) + optional residual add in front, then the per-token quantisation:
//   h = residual ? fp16(residual + x) (written back to residual) : x;  var = mean(float(h)^2);  n = fp16(float(h) * rsqrt(var + eps));
//   y = fp16(float(w) * float(n));  optionally stored;  (xq, s1) = quant(y).   Rows of k elements, k % 8 == 0, contiguous.
template <int VPT, int NT>
__global__ __launch_bounds__(NT) void qqq_rmsnorm_quant_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ residual,
                                                               const _Float16* __restrict__ w, const float eps, _Float16* __restrict__ y,
                                                               int8_t* __restrict__ xq, float* __restrict__ s1, const int K) {
  __shared__ float red_sum[NT / 64], red_max[NT / 64];
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int nvec = K >> 3;
  const size_t off = (size_t)row * K;
  const h8* xr = reinterpret_cast<const h8*>(x + off);
  h8 v[VPT];
  float ss = 0.f;
  if (residual) {
    h8* rr = reinterpret_cast<h8*>(residual + off);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int idx = tid + i * NT;
      if (idx < nvec) {
        const h8 a = xr[idx], b = rr[idx];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i][e] = (_Float16)((float)b[e] + (float)a[e]);
        rr[idx] = v[i];
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int idx = tid + i * NT;
      if (idx < nvec) v[i] = xr[idx];
    }
  }
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    if (tid + i * NT < nvec) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = (float)v[i][e];
        ss = __builtin_fmaf(f, f, ss);
      }
    }
  }
  const float var = qqq_wg_sum<NT>(ss, red_sum) * (1.0f / (float)K);
  const float rs = rsqrtf(var + eps);
  const h8* wr = reinterpret_cast<const h8*>(w);
  h8* yr = y ? reinterpret_cast<h8*>(y + off) : nullptr;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = tid + i * NT;
    if (idx < nvec) {
      const h8 wv = wr[idx];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const _Float16 n = (_Float16)((float)v[i][e] * rs);
        v[i][e] = (_Float16)((float)wv[e] * (float)n);
      }
      if (yr) yr[idx] = v[i];
    }
  }
  qqq_act_quant_row<VPT, NT>(v, nvec, xq + off, s1 + row, red_max);
}

// SiLU·mul (F.silu(gate) * up on fp16), then the per-token quantisation:
//   s = fp16(g / (1 + expf(-g)));  y = fp16(float(s) * float(u));  optionally stored (contiguous [m, I]);  (xq [m, I], s1) = quant(y).
// gate / up rows have their own strides (elements, multiples of 8): one fused gate|up GEMM output (up = gate + I, ld = 2I) or two tensors.
template <int VPT, int NT>
__global__ __launch_bounds__(NT) void qqq_silu_mul_quant_kernel(const _Float16* __restrict__ gate, const int ld_gate,
                                                                const _Float16* __restrict__ up, const int ld_up, _Float16* __restrict__ y,
                                                                int8_t* __restrict__ xq, float* __restrict__ s1, const int I) {
  __shared__ float red_max[NT / 64];
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int nvec = I >> 3;
  const h8* gr = reinterpret_cast<const h8*>(gate + (size_t)row * ld_gate);
  const h8* ur = reinterpret_cast<const h8*>(up + (size_t)row * ld_up);
  h8* yr = y ? reinterpret_cast<h8*>(y + (size_t)row * I) : nullptr;
  h8 v[VPT];
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = tid + i * NT;
    if (idx < nvec) {
      const h8 g = gr[idx], u = ur[idx];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float gf = (float)g[e];
        const _Float16 s = (_Float16)(gf / (1.0f + expf(-gf)));
        v[i][e] = (_Float16)((float)s * (float)u[e]);
      }
      if (yr) yr[idx] = v[i];
    }
  }
  qqq_act_quant_row<VPT, NT>(v, nvec, xq + (size_t)row * I, s1 + row, red_max);
}

#endif  // QQQ_AMD_QQQ_ACT_HIP_H_
