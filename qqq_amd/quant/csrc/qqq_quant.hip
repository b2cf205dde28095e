// qqq_quant.hip -- the one translation unit of libqqq_amd_quant.so: the C-ABI entry points of the GPTQ quantiser
// (qqq_amd/quant/include/qqq_amd_quant.h) over the kernels of qqq_gptq.hip.h, of its act-order / static-groups ops
// (qqq_amd/quant/include/qqq_amd_gptq_order.h) over those of qqq_gptq_order.hip.h, and of the rotation ops
// (qqq_amd/quant/include/qqq_amd_rotate.h, qqq_amd/quant/include_ext/qqq_amd_rotate_k.h) over the kernels of qqq_hadamard.hip.h and qqq_hadamard_k.hip.h,
// and of the smoothing search's fake-quantisation op (qqq_amd/quant/include_ops/qqq_amd_fakequant.h) over those of qqq_fakequant.hip.h.  Built for gfx950 with -ffp-contract=off and no fast-math
// (qqq_amd/build.py, build_quant): the entry points promise bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../../include/qqq_amd.h"  // the return codes
#include "../include/qqq_amd_gptq_order.h"
#include "../include/qqq_amd_quant.h"
#include "../include/qqq_amd_rotate.h"
#include "../include_ext/qqq_amd_rotate_k.h"
#include "../include_ops/qqq_amd_fakequant.h"
#include "qqq_fakequant.hip.h"
#include "qqq_gptq.hip.h"
#include "qqq_gptq_order.hip.h"
#include "qqq_hadamard.hip.h"
#include "qqq_hadamard_k.hip.h"

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
