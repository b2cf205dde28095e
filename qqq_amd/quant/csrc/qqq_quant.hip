// qqq_quant.hip -- the one translation unit of libqqq_amd_quant.so: the C-ABI entry points of the GPTQ quantiser
// (qqq_amd/quant/include/qqq_amd_quant.h) over the kernels of qqq_gptq.hip.h.  Built for gfx950 with -ffp-contract=off and no fast-math
// (qqq_amd/build.py, build_quant): the entry points promise bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../../include/qqq_amd.h"  // the return codes
#include "../include/qqq_amd_quant.h"
#include "qqq_gptq.hip.h"

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
