/*
 * qqq_amd_act.h -- C-ABI of the activation quantisers of a Llama decoder block (exported by libqqq_amd.so, beside include/qqq_amd.h).
 *
 * The fp16 input of a QuantLinear comes out of an RMSNorm (q/k/v, gate/up) or out of SiLU(gate) * up (down_proj).  These entry points
 * produce that activation AND its per-token int8 quantisation in one launch, so the next GEMM (qqq_w4a8_gemm*) reads int8 straight away.
 * The quantisation is bit for bit qqq_dynamic_quant of the fp16 activation (include/qqq_amd.h):
 *   s1[r] = float(fp16(amax_r * (1/127))),  xq[r, j] = clamp(rint(y[r, j] / s1[r]), -128, 127),  an all-zero row gives 0 codes.
 *
 * Conventions are those of include/qqq_amd.h: device pointers on device `dev`, work only ENQUEUED on `stream` (hipStream_t as void*;
 * safe under hipGraph capture), no allocation, no state.  Return codes QQQ_OK / QQQ_ERR_ARG / QQQ_ERR_HIP with a message in
 * qqq_amd_last_error(); bad arguments are rejected before any launch.  m = 0 or k (i) = 0 is a no-op.
 * Row lengths: multiples of 8, at most 65536.  Alignment: fp16 tensors 16 bytes, xq 8 bytes, s1 4 bytes.
 */
#ifndef QQQ_AMD_ACT_H_
#define QQQ_AMD_ACT_H_

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * LlamaRMSNorm (fp16 input, transformers' formula) with an optional residual add in front, then per-token int8 quantisation:
 *   x        fp16 [m,k] row-major
 *   residual fp16 [m,k], in/out, or NULL: h = fp16(residual + x) is written back to residual; NULL: h = x
 *   weight   fp16 [k]
 *   n = fp16(float(h) * rsqrt(mean(float(h)^2) + eps)),  y = fp16(float(weight) * float(n))
 *   y        fp16 [m,k] or NULL (not stored)
 *   xq int8 [m,k], s1 f32 [m]: the quantisation of y
 */
int qqq_rmsnorm_quant(const void* x, void* residual, const void* weight, float eps, void* y, void* xq, void* s1, int m, int k, int dev,
                      void* stream);

/*
 * SiLU(gate) * up (F.silu and `*` on fp16), then per-token int8 quantisation:
 *   gate, up fp16, m rows of i elements with row strides ld_gate, ld_up (elements; >= i, multiples of 8) -- e.g. the two halves of one
 *            fused gate|up GEMM output [m, 2i] (up = gate + i, ld = 2i)
 *   s = fp16(g / (1 + exp(-g))),  y = fp16(float(s) * float(u))
 *   y        fp16 [m,i] contiguous, or NULL (not stored)
 *   xq int8 [m,i], s1 f32 [m]: the quantisation of y
 */
int qqq_silu_mul_quant(const void* gate, int ld_gate, const void* up, int ld_up, void* y, void* xq, void* s1, int m, int i, int dev,
                       void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_ACT_H_ */
