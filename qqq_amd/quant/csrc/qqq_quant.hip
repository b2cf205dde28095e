// qqq_quant.hip -- the one translation unit of libqqq_amd_quant.so: the C-ABI entry points of the GPTQ quantiser
// (qqq_amd/quant/include/qqq_amd_quant.h) over the kernels of qqq_gptq.hip.h, of its act-order / static-groups ops
// (qqq_amd/quant/include/qqq_amd_gptq_order.h) over those of qqq_gptq_order.hip.h, and of the rotation ops
// (qqq_amd/quant/include/qqq_amd_rotate.h, qqq_amd/quant/include/qqq_amd_rotate_k.h) over the kernels of qqq_hadamard.hip.h and qqq_hadamard_k.hip.h,
// of the smoothing search's fake-quantisation op (qqq_amd/quant/include/qqq_amd_fakequant.h) over those of qqq_fakequant.hip.h,
// of the Cholesky factor op (qqq_amd/quant/include/qqq_amd_factor.h) over those of qqq_factor.hip.h,
// and of the Hessian accumulation ops (qqq_amd/quant/include/qqq_amd_hessian.h, qqq_amd/quant/include/qqq_amd_hessian_grouped.h) over the
// kernels of qqq_hessian.hip.h and qqq_hessian_grouped.hip.h.  Built for gfx950 with -ffp-contract=off and no fast-math
// (qqq_amd/build.py, build_quant): the entry points promise bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../../include/qqq_amd.h"  // the return codes
#include "../include/qqq_amd_gptq_order.h"
#include "../include/qqq_amd_quant.h"
#include "../include/qqq_amd_rotate.h"
#include "../include/qqq_amd_rotate_k.h"
#include "../include/qqq_amd_factor.h"
#include "../include/qqq_amd_fakequant.h"
#include "../include/qqq_amd_hessian.h"
#include "../include/qqq_amd_hessian_grouped.h"
#include "qqq_factor.hip.h"
#include "qqq_fakequant.hip.h"
#include "qqq_gptq.hip.h"
#include "qqq_gptq_order.hip.h"
#include "qqq_hadamard.hip.h"
#include "qqq_hadamard_k.hip.h"
#include "qqq_hessian.hip.h"  // (behind qqq_factor.hip.h: it walks the tile triangle with fac_tri)
#include "qqq_hessian_grouped.hip.h"  // (behind qqq_hessian.hip.h: the tile, the operand read and the LDS layout are the dense kernel's)

static thread_local char g_err[512] = "";

static int fail_hip(hipError_t e, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return QQQ_ERR_HIP;
}

struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev && dev >= 0) changed = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
};

static bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

extern "C" int qqq_quant_abi_version(void) { return QQQ_AMD_QUANT_ABI_VERSION; }
extern "C" const char* qqq_quant_last_error(void) { return g_err; }

extern "C" int qqq_gptq_scales(const void* W, int ldw, int rows, int cols, int grouped, int mse, void* scale_out, int dev, void* stream) {
  g_err[0] = 0;
  if (rows < 1 || cols < 1 || cols > 1048576 || ldw < cols) {
    snprintf(g_err, sizeof(g_err), "qqq_gptq_scales: bad shape rows=%d cols=%d ldw=%d (need rows >= 1, 1 <= cols <= 1048576, ldw >= cols)", rows,
             cols, ldw);
    return QQQ_ERR_ARG;
  }
  if ((grouped != 0 && grouped != 1) || (mse != 0 && mse != 1)) {
    snprintf(g_err, sizeof(g_err), "qqq_gptq_scales: grouped=%d and mse=%d must each be 0 or 1", grouped, mse);
    return QQQ_ERR_ARG;
  }
  if (!W || !scale_out || misaligned(W, 4) || misaligned(scale_out, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_gptq_scales: bad argument (W and scale_out must be non-NULL and 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  qqq_gptq_scales_args a;
  a.W = static_cast<const float*>(W);
  a.out = static_cast<float*>(scale_out);
  a.ldw = ldw;
  a.rows = rows;
  a.cols = cols;
  a.grouped = grouped;
  a.mse = mse;
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (cols <= GPTQ_SC_NARROW)
    hipLaunchKernelGGL(qqq_gptq_scales_kernel<64>, dim3((rows + 3) / 4), dim3(GPTQ_SC_NT), 0, st, a);
  else
    hipLaunchKernelGGL(qqq_gptq_scales_kernel<GPTQ_SC_NT>, dim3(rows), dim3(GPTQ_SC_NT), 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_gptq_scales_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_gptq_block(const void* W1, int ldw, const void* Hinv1, int ldh, const void* scale, int rows, int count, int grouped,
                              void* Q1, int ldq, void* Err1, int lde, int dev, void* stream) {
  g_err[0] = 0;
  if (count != 64 && count != 128) {
    snprintf(g_err, sizeof(g_err), "qqq_gptq_block: count=%d is not one of 64, 128", count);
    return QQQ_ERR_ARG;
  }
  if (rows < 1 || ldw < count || ldh < count || ldq < count || lde < count) {
    snprintf(g_err, sizeof(g_err), "qqq_gptq_block: bad shape rows=%d ldw=%d ldh=%d ldq=%d lde=%d (need rows >= 1 and every stride >= count=%d)",
             rows, ldw, ldh, ldq, lde, count);
    return QQQ_ERR_ARG;
  }
  if (grouped != 0 && grouped != 1) {
    snprintf(g_err, sizeof(g_err), "qqq_gptq_block: grouped=%d must be 0 or 1", grouped);
    return QQQ_ERR_ARG;
  }
  if (!W1 || !Hinv1 || !scale || !Q1 || !Err1 || misaligned(W1, 4) || misaligned(Hinv1, 4) || misaligned(scale, 4) || misaligned(Q1, 4) ||
      misaligned(Err1, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_gptq_block: bad argument (every pointer must be non-NULL and 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  qqq_gptq_block_args a;
  a.W1 = static_cast<const float*>(W1);
  a.Hinv1 = static_cast<const float*>(Hinv1);
  a.scale = static_cast<const float*>(scale);
  a.Q1 = static_cast<float*>(Q1);
  a.Err1 = static_cast<float*>(Err1);
  a.ldw = ldw;
  a.ldh = ldh;
  a.ldq = ldq;
  a.lde = lde;
  a.rows = rows;
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((rows + GPTQ_ROWS - 1) / GPTQ_ROWS);
  if (count == 64 && grouped)
    hipLaunchKernelGGL((qqq_gptq_block_kernel<64, true>), grid, dim3(GPTQ_NT), 0, st, a);
  else if (count == 64)
    hipLaunchKernelGGL((qqq_gptq_block_kernel<64, false>), grid, dim3(GPTQ_NT), 0, st, a);
  else if (grouped)
    hipLaunchKernelGGL((qqq_gptq_block_kernel<128, true>), grid, dim3(GPTQ_NT), 0, st, a);
  else
    hipLaunchKernelGGL((qqq_gptq_block_kernel<128, false>), grid, dim3(GPTQ_NT), 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_gptq_block_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_gptq_group_scales(const void* W, int ldw, int rows, int cols, int mse, void* scales_out, int lds, int dev, void* stream) {
  g_err[0] = 0;
  if (rows < 1 || cols < 128 || cols > 1048576 || cols % 128 != 0 || ldw < cols || lds < cols / 128) {
    snprintf(g_err, sizeof(g_err),
             "qqq_gptq_group_scales: bad shape rows=%d cols=%d ldw=%d lds=%d (need rows >= 1, cols a multiple of 128 in 128 ... 1048576, ldw >= "
             "cols, lds >= cols / 128)",
             rows, cols, ldw, lds);
    return QQQ_ERR_ARG;
  }
  if (mse != 0 && mse != 1) {
    snprintf(g_err, sizeof(g_err), "qqq_gptq_group_scales: mse=%d must be 0 or 1", mse);
    return QQQ_ERR_ARG;
  }
  if (!W || !scales_out || misaligned(W, 4) || misaligned(scales_out, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_gptq_group_scales: bad argument (W and scales_out must be non-NULL and 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  qqq_gptq_group_scales_args a;
  a.W = static_cast<const float*>(W);
  a.out = static_cast<float*>(scales_out);
  a.ldw = ldw;
  a.lds = lds;
  a.groups = cols / 128;
  a.pairs = static_cast<long long>(rows) * a.groups;
  a.mse = mse;
  const long long grid = (a.pairs + GPTQ_SC_NT / 64 - 1) / (GPTQ_SC_NT / 64);
  if (grid > 0x7fffffffLL) {
    snprintf(g_err, sizeof(g_err), "qqq_gptq_group_scales: rows=%d x cols=%d is more than one launch holds", rows, cols);
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_gptq_group_scales_kernel, dim3(static_cast<unsigned>(grid)), dim3(GPTQ_SC_NT), 0, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_gptq_group_scales_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_gptq_block_cols(const void* W1, int ldw, const void* Hinv1, int ldh, const void* scales, int lds, int groups,
                                   const void* gidx, int rows, int count, void* Q1, int ldq, void* Err1, int lde, int dev, void* stream) {
  g_err[0] = 0;
  if (count != 64 && count != 128) {
    snprintf(g_err, sizeof(g_err), "qqq_gptq_block_cols: count=%d is not one of 64, 128", count);
    return QQQ_ERR_ARG;
  }
  if (rows < 1 || groups < 1 || lds < groups || ldw < count || ldh < count || ldq < count || lde < count) {
    snprintf(g_err, sizeof(g_err),
             "qqq_gptq_block_cols: bad shape rows=%d groups=%d lds=%d ldw=%d ldh=%d ldq=%d lde=%d (need rows >= 1, groups >= 1, lds >= groups "
             "and every other stride >= count=%d)",
             rows, groups, lds, ldw, ldh, ldq, lde, count);
    return QQQ_ERR_ARG;
  }
  if (!W1 || !Hinv1 || !scales || !gidx || !Q1 || !Err1 || misaligned(W1, 4) || misaligned(Hinv1, 4) || misaligned(scales, 4) ||
      misaligned(gidx, 4) || misaligned(Q1, 4) || misaligned(Err1, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_gptq_block_cols: bad argument (every pointer must be non-NULL and 4-byte aligned)");
    return QQQ_ERR_ARG;
  }
  qqq_gptq_block_cols_args a;
  a.W1 = static_cast<const float*>(W1);
  a.Hinv1 = static_cast<const float*>(Hinv1);
  a.scales = static_cast<const float*>(scales);
  a.gidx = static_cast<const int*>(gidx);
  a.Q1 = static_cast<float*>(Q1);
  a.Err1 = static_cast<float*>(Err1);
  a.ldw = ldw;
  a.ldh = ldh;
  a.lds = lds;
  a.ldq = ldq;
  a.lde = lde;
  a.rows = rows;
  a.groups = groups;
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((rows + GPTQ_ROWS - 1) / GPTQ_ROWS);
  if (count == 64)
    hipLaunchKernelGGL(qqq_gptq_block_cols_kernel<64>, grid, dim3(GPTQ_NT), 0, st, a);
  else
    hipLaunchKernelGGL(qqq_gptq_block_cols_kernel<128>, grid, dim3(GPTQ_NT), 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_gptq_block_cols_kernel launch");
  return QQQ_OK;
}

template <typename T, bool VEC>
static void hadamard_launch(const qqq_hadamard_args& a, hipStream_t st) {
  // the tile holds whole blocks: 2048 elements up to n = 2048, then the block itself
  if (a.n <= 2048)
    hipLaunchKernelGGL((qqq_hadamard_kernel<T, VEC, 11>), dim3(static_cast<unsigned>((a.units + 255) / 256)), dim3(256), 0, st, a);
  else if (a.n == 4096)
    hipLaunchKernelGGL((qqq_hadamard_kernel<T, VEC, 12>), dim3(static_cast<unsigned>((a.units + 511) / 512)), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((qqq_hadamard_kernel<T, VEC, 13>), dim3(static_cast<unsigned>((a.units + 1023) / 1024)), dim3(1024), 0, st, a);
}

extern "C" int qqq_hadamard_rows(const void* X, int ldx, void* Y, int ldy, int rows, int cols, int n, const void* sign, int dtype, int dev,
                                 void* stream) {
  g_err[0] = 0;
  if (dtype != 0 && dtype != 1) {
    snprintf(g_err, sizeof(g_err), "qqq_hadamard_rows: dtype=%d is not 0 (fp16) or 1 (f32)", dtype);
    return QQQ_ERR_ARG;
  }
  if (n < 2 || n > HAD_MAX_N || (n & (n - 1)) != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_hadamard_rows: n=%d is not a power of two in 2 ... %d", n, HAD_MAX_N);
    return QQQ_ERR_ARG;
  }
  if (rows < 1 || cols < n || cols % n != 0 || ldx < cols || ldy < cols) {
    snprintf(g_err, sizeof(g_err), "qqq_hadamard_rows: bad shape rows=%d cols=%d ldx=%d ldy=%d (need rows >= 1, cols a positive multiple of n=%d, both strides >= cols)",
             rows, cols, ldx, ldy, n);
    return QQQ_ERR_ARG;
  }
  const uintptr_t es = dtype == 0 ? 2 : 4;
  if (!X || !Y || misaligned(X, es) || misaligned(Y, es)) {
    snprintf(g_err, sizeof(g_err), "qqq_hadamard_rows: bad argument (X and Y must be non-NULL and aligned to their element, %d bytes)", static_cast<int>(es));
    return QQQ_ERR_ARG;
  }
  const uintptr_t x0 = reinterpret_cast<uintptr_t>(X), y0 = reinterpret_cast<uintptr_t>(Y);
  const uintptr_t xspan = (static_cast<uintptr_t>(rows - 1) * ldx + cols) * es, yspan = (static_cast<uintptr_t>(rows - 1) * ldy + cols) * es;
  if (x0 == y0 ? ldx != ldy : (x0 < y0 + yspan && y0 < x0 + xspan)) {
    snprintf(g_err, sizeof(g_err), "qqq_hadamard_rows: X and Y overlap (only Y == X with ldy == ldx, in place, is allowed)");
    return QQQ_ERR_ARG;
  }
  qqq_hadamard_args a;
  a.X = X;
  a.Y = Y;
  a.sign = static_cast<const signed char*>(sign);
  a.ldx = ldx;
  a.ldy = ldy;
  a.run = n < HAD_RUN ? n : HAD_RUN;
  a.units_per_row = cols / a.run;
  a.units = static_cast<long long>(rows) * a.units_per_row;
  a.n = n;
  a.log2n = 0;
  while ((1 << a.log2n) < n) ++a.log2n;
  a.d = static_cast<double>(sqrtf(static_cast<float>(n)));
  a.rd = 1.0 / a.d;
  if ((a.units + 255) / 256 > 0x7fffffffLL) {
    snprintf(g_err, sizeof(g_err), "qqq_hadamard_rows: rows=%d x cols=%d is more than one launch holds", rows, cols);
    return QQQ_ERR_ARG;
  }
  // 16-byte loads and stores of a run (and one 8-byte load of its signs) where every run of both matrices is 16-byte aligned and the
  // sign vector 8-byte; the bits do not depend on it
  const uintptr_t per16 = 16 / es;
  const bool vec = a.run == HAD_RUN && !misaligned(X, 16) && !misaligned(Y, 16) && ldx % per16 == 0 && ldy % per16 == 0 && !misaligned(sign, 8);
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == 0 && vec)
    hadamard_launch<_Float16, true>(a, st);
  else if (dtype == 0)
    hadamard_launch<_Float16, false>(a, st);
  else if (vec)
    hadamard_launch<float, true>(a, st);
  else
    hadamard_launch<float, false>(a, st);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_hadamard_kernel launch");
  return QQQ_OK;
}

template <typename T, bool VEC>
static void hadamard_k_launch(const qqq_hadamard_k_args& a, unsigned grid, hipStream_t st) {
  // the workgroup holds whole blocks: as many as fit 256 runs up to n = 2048, then the block itself
  if (a.n <= 2048)
    hipLaunchKernelGGL((qqq_hadamard_k_kernel<T, VEC, 11>), dim3(grid), dim3(256), 0, st, a);
  else if (a.n <= 4096)
    hipLaunchKernelGGL((qqq_hadamard_k_kernel<T, VEC, 12>), dim3(grid), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((qqq_hadamard_k_kernel<T, VEC, 13>), dim3(grid), dim3(1024), 0, st, a);
}

extern "C" int qqq_hadamard_rows_k(const void* X, int ldx, void* Y, int ldy, int rows, int cols, int K, int m, const void* table,
                                   const void* sign, int dtype, int dev, void* stream) {
  g_err[0] = 0;
  if (dtype != 0 && dtype != 1) {
    snprintf(g_err, sizeof(g_err), "qqq_hadamard_rows_k: dtype=%d is not 0 (fp16) or 1 (f32)", dtype);
    return QQQ_ERR_ARG;
  }
  if (K < 4 || K > HAD_K_MAX || K % 4 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_hadamard_rows_k: K=%d is not a multiple of 4 in 4 ... %d", K, HAD_K_MAX);
    return QQQ_ERR_ARG;
  }
  if (m < 1 || m > HAD_MAX_N / K || (m & (m - 1)) != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_hadamard_rows_k: m=%d is not a power of two with K * m = %d * m <= %d", m, K, HAD_MAX_N);
    return QQQ_ERR_ARG;
  }
  const int n = K * m;
  if (rows < 1 || cols < n || cols % n != 0 || ldx < cols || ldy < cols) {
    snprintf(g_err, sizeof(g_err),
             "qqq_hadamard_rows_k: bad shape rows=%d cols=%d ldx=%d ldy=%d (need rows >= 1, cols a positive multiple of n=%d, both strides >= cols)",
             rows, cols, ldx, ldy, n);
    return QQQ_ERR_ARG;
  }
  const uintptr_t es = dtype == 0 ? 2 : 4;
  if (!X || !Y || !table || misaligned(X, es) || misaligned(Y, es)) {
    snprintf(g_err, sizeof(g_err),
             "qqq_hadamard_rows_k: bad argument (X, Y and table must be non-NULL, X and Y aligned to their element, %d bytes)", static_cast<int>(es));
    return QQQ_ERR_ARG;
  }
  const uintptr_t x0 = reinterpret_cast<uintptr_t>(X), y0 = reinterpret_cast<uintptr_t>(Y);
  const uintptr_t xspan = (static_cast<uintptr_t>(rows - 1) * ldx + cols) * es, yspan = (static_cast<uintptr_t>(rows - 1) * ldy + cols) * es;
  if (x0 == y0 ? ldx != ldy : (x0 < y0 + yspan && y0 < x0 + xspan)) {
    snprintf(g_err, sizeof(g_err), "qqq_hadamard_rows_k: X and Y overlap (only Y == X with ldy == ldx, in place, is allowed)");
    return QQQ_ERR_ARG;
  }
  qqq_hadamard_k_args a;
  a.X = X;
  a.Y = Y;
  a.sign = static_cast<const signed char*>(sign);
  a.table = static_cast<const signed char*>(table);
  a.ldx = ldx;
  a.ldy = ldy;
  a.blocks_per_row = cols / n;
  a.blocks = static_cast<long long>(rows) * a.blocks_per_row;
  a.run = n % HAD_RUN == 0 ? HAD_RUN : HAD_RUN / 2;  // K is a multiple of 4: n % 8 is 0 or 4
  a.group = n <= 2048 ? 256 * a.run / n : 1;
  a.n = n;
  a.K = K;
  a.m = m;
  a.log2m = 0;
  while ((1 << a.log2m) < m) ++a.log2m;
  a.uniform = m % 8 == 0 && (a.group * m) % 64 == 0;
  a.d = static_cast<double>(sqrtf(static_cast<float>(n)));
  a.rd = 1.0 / a.d;
  const long long grid = (a.blocks + a.group - 1) / a.group;
  if (grid > 0x7fffffffLL) {
    snprintf(g_err, sizeof(g_err), "qqq_hadamard_rows_k: rows=%d x cols=%d is more than one launch holds", rows, cols);
    return QQQ_ERR_ARG;
  }
  // 16-byte loads and stores of a run (and one 8-byte load of its signs) where every run of both matrices is 16-byte aligned and the
  // sign vector 8-byte; the bits do not depend on it
  const uintptr_t per16 = 16 / es;
  const bool vec = a.run == HAD_RUN && !misaligned(X, 16) && !misaligned(Y, 16) && ldx % per16 == 0 && ldy % per16 == 0 && !misaligned(sign, 8);
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned blocks = static_cast<unsigned>(grid);
  if (dtype == 0 && vec)
    hadamard_k_launch<_Float16, true>(a, blocks, st);
  else if (dtype == 0)
    hadamard_k_launch<_Float16, false>(a, blocks, st);
  else if (vec)
    hadamard_k_launch<float, true>(a, blocks, st);
  else
    hadamard_k_launch<float, false>(a, blocks, st);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_hadamard_k_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_fake_quant_rows(const void* X, int ldx, void* Y, int ldy, int rows, int cols, const void* col_scale, int bits, int group,
                                   int divide, int dev, void* stream) {
  g_err[0] = 0;
  if (bits != 4 && bits != 8) {
    snprintf(g_err, sizeof(g_err), "qqq_fake_quant_rows: bits=%d is not one of 4, 8", bits);
    return QQQ_ERR_ARG;
  }
  if (group != 0 && group != 128) {
    snprintf(g_err, sizeof(g_err), "qqq_fake_quant_rows: group=%d is not 0 (one scale per row) or 128", group);
    return QQQ_ERR_ARG;
  }
  if (divide != 0 && divide != 1) {
    snprintf(g_err, sizeof(g_err), "qqq_fake_quant_rows: divide=%d must be 0 or 1", divide);
    return QQQ_ERR_ARG;
  }
  if (rows < 1 || cols < FQ_UNIT || cols > (1 << 30) || cols % FQ_UNIT != 0 || ldx < cols || ldy < cols || ldx % FQ_UNIT != 0 || ldy % FQ_UNIT != 0) {
    snprintf(g_err, sizeof(g_err),
             "qqq_fake_quant_rows: bad shape rows=%d cols=%d ldx=%d ldy=%d (need rows >= 1, cols a multiple of 8 in 8 ... 2^30, both strides "
             ">= cols and multiples of 8)",
             rows, cols, ldx, ldy);
    return QQQ_ERR_ARG;
  }
  if (group == 128 && cols % 128 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_fake_quant_rows: cols=%d is no multiple of group=128", cols);
    return QQQ_ERR_ARG;
  }
  if (!X || !Y || misaligned(X, 16) || misaligned(Y, 16) || misaligned(col_scale, 16)) {
    snprintf(g_err, sizeof(g_err), "qqq_fake_quant_rows: bad argument (X and Y must be non-NULL, X, Y and col_scale 16-byte aligned)");
    return QQQ_ERR_ARG;
  }
  const uintptr_t x0 = reinterpret_cast<uintptr_t>(X), y0 = reinterpret_cast<uintptr_t>(Y);
  const uintptr_t xspan = (static_cast<uintptr_t>(rows - 1) * ldx + cols) * 2, yspan = (static_cast<uintptr_t>(rows - 1) * ldy + cols) * 2;
  if (x0 == y0 ? ldx != ldy : (x0 < y0 + yspan && y0 < x0 + xspan)) {
    snprintf(g_err, sizeof(g_err), "qqq_fake_quant_rows: X and Y overlap (only Y == X with ldy == ldx, in place, is allowed)");
    return QQQ_ERR_ARG;
  }
  qqq_fake_quant_args a;
  a.X = static_cast<const _Float16*>(X);
  a.Y = static_cast<_Float16*>(Y);
  a.c = static_cast<const _Float16*>(col_scale);
  a.ldx = ldx;
  a.ldy = ldy;
  a.units_per_row = cols / FQ_UNIT;
  a.units = static_cast<long long>(rows) * a.units_per_row;
  a.divide = divide;
  a.qmax = bits == 8 ? 127.f : 7.f;
  const long long grid = group ? (a.units + FQ_NT - 1) / FQ_NT : rows;
  if (grid > 0x7fffffffLL) {
    snprintf(g_err, sizeof(g_err), "qqq_fake_quant_rows: rows=%d x cols=%d is more than one launch holds", rows, cols);
    return QQQ_ERR_ARG;
  }
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 g(static_cast<unsigned>(grid)), b(FQ_NT);
  if (group)
    hipLaunchKernelGGL(qqq_fake_quant_group_kernel, g, b, 0, st, a);
  else if (a.units_per_row <= FQ_NT)  // the row is read once where its units fit the registers of its workgroup
    hipLaunchKernelGGL(qqq_fake_quant_row_kernel<1>, g, b, 0, st, a);
  else if (a.units_per_row <= 2 * FQ_NT)
    hipLaunchKernelGGL(qqq_fake_quant_row_kernel<2>, g, b, 0, st, a);
  else if (a.units_per_row <= 4 * FQ_NT)
    hipLaunchKernelGGL(qqq_fake_quant_row_kernel<4>, g, b, 0, st, a);
  else if (a.units_per_row <= FQ_MAX_UPT * FQ_NT)
    hipLaunchKernelGGL(qqq_fake_quant_row_kernel<FQ_MAX_UPT>, g, b, 0, st, a);
  else
    hipLaunchKernelGGL(qqq_fake_quant_row_kernel<0>, g, b, 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_fake_quant_rows kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_upper_factor_work(int n, long long* bytes) {
  g_err[0] = 0;
  if (n < 64 || n > 32768 || n % 64 != 0 || !bytes) {
    snprintf(g_err, sizeof(g_err), "qqq_upper_factor_work: n=%d is not a multiple of 64 in 64 ... 32768, or bytes is NULL", n);
    return QQQ_ERR_ARG;
  }
  *bytes = (static_cast<long long>(n) * n + static_cast<long long>(n) * FAC_BLOCK) * 4;  // the running matrix, and the strip T
  return QQQ_OK;
}

template <bool BT, bool NEG>
static void factor_gemm(const qqq_factor_gemm_args& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((qqq_factor_gemm_kernel<BT, NEG>), grid, dim3(FAC_NT), 0, st, a);
}

extern "C" int qqq_upper_factor(const void* H, int ldh, void* U, int ldu, int n, void* work, void* info, int dev, void* stream) {
  g_err[0] = 0;
  if (n < 64 || n > 32768 || n % 64 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_upper_factor: n=%d is not a multiple of 64 in 64 ... 32768", n);
    return QQQ_ERR_ARG;
  }
  if (ldh < n || ldu < n || ldh % 4 != 0 || ldu % 4 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_upper_factor: bad strides ldh=%d ldu=%d (need both >= n=%d and multiples of 4)", ldh, ldu, n);
    return QQQ_ERR_ARG;
  }
  if (!H || !U || !work || !info || misaligned(H, 16) || misaligned(U, 16) || misaligned(work, 16) || misaligned(info, 4)) {
    snprintf(g_err, sizeof(g_err), "qqq_upper_factor: bad argument (H, U, work and info must be non-NULL, H, U and work 16-byte aligned, info 4-byte)");
    return QQQ_ERR_ARG;
  }
  const uintptr_t h0 = reinterpret_cast<uintptr_t>(H), u0 = reinterpret_cast<uintptr_t>(U), w0 = reinterpret_cast<uintptr_t>(work),
                  i0 = reinterpret_cast<uintptr_t>(info);
  const uintptr_t hspan = (static_cast<uintptr_t>(n - 1) * ldh + n) * 4, uspan = (static_cast<uintptr_t>(n - 1) * ldu + n) * 4;
  const uintptr_t wspan = (static_cast<uintptr_t>(n) * n + static_cast<uintptr_t>(n) * FAC_BLOCK) * 4;
  auto meet = [](uintptr_t p, uintptr_t ps, uintptr_t q, uintptr_t qs) { return p < q + qs && q < p + ps; };
  if (meet(h0, hspan, u0, uspan) || meet(h0, hspan, w0, wspan) || meet(u0, uspan, w0, wspan) || meet(i0, 4, h0, hspan) ||
      meet(i0, 4, u0, uspan) || meet(i0, 4, w0, wspan)) {
    snprintf(g_err, sizeof(g_err), "qqq_upper_factor: H, U, work and info overlap (the four must be disjoint)");
    return QQQ_ERR_ARG;
  }
  const float* Hp = static_cast<const float*>(H);
  float* Up = static_cast<float*>(U);
  float* W = static_cast<float*>(work);
  float* T = W + static_cast<long long>(n) * n;
  const long long ldw = n;
  DeviceGuard guard(dev);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int tiles = n / FAC_TILE;
  if (tiles > 1) {
    qqq_factor_zero_args z;
    z.U = Up;
    z.ldu = ldu;
    hipLaunchKernelGGL(qqq_factor_zero_kernel, dim3(static_cast<unsigned>(tiles * (tiles - 1) / 2)), dim3(FAC_NT), 0, st, z);
  }
  // the factorisation: diagonal blocks of 128 from the end, a first block of 64 where n is an odd multiple of 64
  bool first = true;
  for (int c1 = n; c1 > 0;) {
    const int bw = c1 >= FAC_BLOCK ? FAC_BLOCK : FAC_TILE, c0 = c1 - bw, t0 = c0 / FAC_TILE;
    const float* src = first ? Hp : W;
    const long long lds = first ? ldh : ldw;
    qqq_factor_diag_args d;
    d.src = src + c0 * lds + c0;
    d.U = Up + static_cast<long long>(c0) * ldu + c0;
    d.info = static_cast<int*>(info);
    d.lds = lds;
    d.ldu = ldu;
    d.base = c0;
    d.first = first ? 1 : 0;
    if (bw == FAC_BLOCK)
      hipLaunchKernelGGL(qqq_factor_diag_kernel<FAC_BLOCK>, dim3(1), dim3(FAC_NT), 0, st, d);
    else
      hipLaunchKernelGGL(qqq_factor_diag_kernel<FAC_TILE>, dim3(1), dim3(FAC_NT), 0, st, d);
    if (t0 > 0) {
      qqq_factor_gemm_args g;
      g.A = src + c0;  // panel: U_iJ = src_iJ . U_JJ^T
      g.lda = lds;
      g.B = d.U;
      g.ldb = ldu;
      g.Cin = nullptr;
      g.ldcin = 0;
      g.C = Up + c0;
      g.ldc = ldu;
      g.K = bw;
      g.tri_grid = 0;
      g.tri_k = 0;
      factor_gemm<true, false>(g, dim3(t0, bw / FAC_TILE), st);
      g.A = Up + c0;  // update: W_ik = src_ik - U_iJ . U_kJ^T, i <= k < J
      g.lda = ldu;
      g.B = Up + c0;
      g.ldb = ldu;
      g.Cin = src;
      g.ldcin = lds;
      g.C = W;
      g.ldc = ldw;
      g.tri_grid = 1;
      factor_gemm<true, true>(g, dim3(static_cast<unsigned>(t0 * (t0 + 1) / 2)), st);
    }
    first = false;
    c1 = c0;
  }
  // the inverse: block columns ascending (the first has nothing above it)
  for (int c0 = n % FAC_BLOCK ? FAC_TILE : FAC_BLOCK; c0 < n; c0 += FAC_BLOCK) {
    const int t0 = c0 / FAC_TILE;
    qqq_factor_gemm_args g;
    g.A = Up + c0;  // T = R_{0:c0, J} . U_JJ
    g.lda = ldu;
    g.B = Up + static_cast<long long>(c0) * ldu + c0;
    g.ldb = ldu;
    g.Cin = nullptr;
    g.ldcin = 0;
    g.C = T;
    g.ldc = FAC_BLOCK;
    g.K = FAC_BLOCK;
    g.tri_grid = 0;
    g.tri_k = 0;
    factor_gemm<false, false>(g, dim3(t0, FAC_BLOCK / FAC_TILE), st);
    g.A = Up;  // U_{0:c0, J} = - U_{0:c0, 0:c0} . T
    g.B = T;
    g.ldb = FAC_BLOCK;
    g.C = Up + c0;
    g.ldc = ldu;
    g.K = c0;
    g.tri_k = 1;
    factor_gemm<false, true>(g, dim3(t0, FAC_BLOCK / FAC_TILE), st);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_upper_factor launch chain");
  return QQQ_OK;
}

extern "C" int qqq_hessian_update(void* H, int ldh, const void* X, int ldx, int tokens, int n, float alpha, float beta, int dev, void* stream) {
  g_err[0] = 0;
  if (n < 64 || n > 32768 || n % 64 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_hessian_update: n=%d is not a multiple of 64 in 64 ... 32768", n);
    return QQQ_ERR_ARG;
  }
  if (tokens < 1) {
    snprintf(g_err, sizeof(g_err), "qqq_hessian_update: tokens=%d must be at least 1", tokens);
    return QQQ_ERR_ARG;
  }
  if (ldh < n || ldx < n || ldh % 4 != 0 || ldx % 8 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_hessian_update: bad strides ldh=%d ldx=%d (need both >= n=%d, ldh a multiple of 4, ldx of 8)", ldh, ldx, n);
    return QQQ_ERR_ARG;
  }
  if (!H || !X || misaligned(H, 16) || misaligned(X, 16)) {
    snprintf(g_err, sizeof(g_err), "qqq_hessian_update: bad argument (H and X must be non-NULL and 16-byte aligned)");
    return QQQ_ERR_ARG;
  }
  const uintptr_t h0 = reinterpret_cast<uintptr_t>(H), x0 = reinterpret_cast<uintptr_t>(X);
  const uintptr_t hspan = (static_cast<uintptr_t>(n - 1) * ldh + n) * 4, xspan = (static_cast<uintptr_t>(tokens - 1) * ldx + n) * 2;
  if (h0 < x0 + xspan && x0 < h0 + hspan) {
    snprintf(g_err, sizeof(g_err), "qqq_hessian_update: H and X overlap (the two must be disjoint)");
    return QQQ_ERR_ARG;
  }
  qqq_hessian_args a;
  a.H = static_cast<float*>(H);
  a.X = static_cast<const _Float16*>(X);
  a.ldh = ldh;
  a.ldx = ldx;
  a.tokens = tokens;
  a.n = n;
  a.nb = (n + HES_TILE - 1) / HES_TILE;
  a.ntiles = a.nb * (a.nb + 1) / 2;  // (at most 256 * 257 / 2)
  a.alpha = alpha;
  a.beta = beta;
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_hessian_kernel, dim3(static_cast<unsigned>(a.ntiles)), dim3(HES_NT), 0, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_hessian_kernel launch");
  return QQQ_OK;
}

extern "C" int qqq_hessian_update_grouped(void* H, size_t lde, int ldh, const void* X, int ldx, const void* offsets, const void* order,
                                          const void* alpha, const void* beta, int P, int R, int E, int n, int a_div, int dev, void* stream) {
  g_err[0] = 0;
  if (n < 64 || n > 32768 || n % 64 != 0) {
    snprintf(g_err, sizeof(g_err), "qqq_hessian_update_grouped: n=%d is not a multiple of 64 in 64 ... 32768", n);
    return QQQ_ERR_ARG;
  }
  if (E < 1 || E > 256) {
    snprintf(g_err, sizeof(g_err), "qqq_hessian_update_grouped: E=%d is not in 1 ... 256", E);
    return QQQ_ERR_ARG;
  }
  if (P < 0 || P > 2097152 || a_div < 1 || R < 0 || static_cast<long long>(R) * a_div < P) {
    snprintf(g_err, sizeof(g_err), "qqq_hessian_update_grouped: bad routing shape P=%d R=%d a_div=%d (need 0 <= P <= 2097152, a_div >= 1, R >= ceil(P / a_div))",
             P, R, a_div);
    return QQQ_ERR_ARG;
  }
  if (ldh < n || ldx < n || ldh % 4 != 0 || ldx % 8 != 0 || lde < static_cast<size_t>(n) * ldh || lde % 4 != 0 || lde > (size_t{1} << 40)) {
    snprintf(g_err, sizeof(g_err),
             "qqq_hessian_update_grouped: bad strides lde=%zu ldh=%d ldx=%d (need ldh and ldx >= n=%d, ldh a multiple of 4, ldx of 8, lde >= n * ldh "
             "and a multiple of 4)",
             lde, ldh, ldx, n);
    return QQQ_ERR_ARG;
  }
  if (!H || !X || !offsets || !order || !alpha || !beta || misaligned(H, 16) || misaligned(X, 16) || misaligned(offsets, 4) || misaligned(order, 4) ||
      misaligned(alpha, 4) || misaligned(beta, 4)) {
    snprintf(g_err, sizeof(g_err),
             "qqq_hessian_update_grouped: bad argument (every pointer must be non-NULL, H and X 16-byte aligned, offsets, order, alpha and beta 4-byte)");
    return QQQ_ERR_ARG;
  }
  const uintptr_t h0 = reinterpret_cast<uintptr_t>(H), x0 = reinterpret_cast<uintptr_t>(X);
  const uintptr_t hspan = (static_cast<uintptr_t>(E - 1) * lde + static_cast<uintptr_t>(n - 1) * ldh + n) * 4;
  const uintptr_t xspan = R > 0 ? (static_cast<uintptr_t>(R - 1) * ldx + n) * 2 : 0;
  if (h0 < x0 + xspan && x0 < h0 + hspan) {
    snprintf(g_err, sizeof(g_err), "qqq_hessian_update_grouped: H and X overlap (the two must be disjoint)");
    return QQQ_ERR_ARG;
  }
  if (P == 0) return QQQ_OK;  // no pair, no expert with a row: nothing to do
  qqq_hessian_grouped_args a;
  a.H = static_cast<float*>(H);
  a.X = static_cast<const _Float16*>(X);
  a.offsets = static_cast<const int*>(offsets);
  a.order = static_cast<const int*>(order);
  a.alpha = static_cast<const float*>(alpha);
  a.beta = static_cast<const float*>(beta);
  a.lde = static_cast<long long>(lde);
  a.ldh = ldh;
  a.ldx = ldx;
  a.P = P;
  a.R = R;
  a.n = n;
  a.a_div = a_div;
  const int nb = (n + HES_TILE - 1) / HES_TILE;
  a.ntiles = nb * (nb + 1) / 2;
  a.work = E * a.ntiles;  // the launch follows (E, n) alone: a captured call replays with another routing
  DeviceGuard guard(dev);
  hipLaunchKernelGGL(qqq_hessian_grouped_kernel, dim3(static_cast<unsigned>(a.work)), dim3(HES_NT), 0, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "qqq_hessian_grouped_kernel launch");
  return QQQ_OK;
}
