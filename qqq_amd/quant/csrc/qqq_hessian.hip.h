// qqq_hessian.hip.h -- the kernel of qqq_hessian_update (qqq_amd/quant/include/qqq_amd_hessian.h): GPTQ's running Hessian
//   H <- f32(f32(alpha H) + f32(beta S)),  S = X^T X,  X fp16 [tokens, n]
// as a symmetric rank-k update on the fp16 matrix path.  Part of the single translation unit qqq_quant.hip (floating-point contraction
// off: the epilogue's two products and its sum are three roundings).
//
//   qqq_hessian_kernel   one workgroup of four waves per 128 x 128 tile (bi <= bj) of the upper block triangle; only those are launched.
//     order     the linear index runs through the triangle column by column (p = bj (bj + 1) / 2 + bi, fac_tri), so neighbours share the
//               column panel bj of X; workgroup b runs on XCD b % 8 and every XCD takes one contiguous run of that order (the mapping of
//               the GEMM kernels of libqqq_amd.so), so the panels a run shares stay in one L2.
//     staging   the token loop runs in stages of HES_TS = 32 tokens.  X[t0 : t0 + 32, panel] of the row panel bi and the column panel bj
//               goes row-major into LDS with 16-byte global loads (two per thread and panel); rows >= tokens and columns >= n are
//               zero-filled in LDS (never loaded), so the MFMA loop has no tail.  A diagonal tile stages one panel and reads both operands
//               from it.  Two buffers: the loads of stage s + 1 are issued before the MFMAs of stage s and stored behind them, one
//               barrier a stage.
//     operands  the reduction index is X's ROW index, so both operands of v_mfma_f32_32x32x16_f16 are column reads of the staged panel:
//               ds_read_b64_tr_b16 (four tokens x sixteen columns per 16-lane group, column-major), two reads per 32 x 16 operand.  The row
//               stride is 128 + 32 halves = 320 bytes, 64 mod 256: the four token rows a half-wave reads lie in four disjoint quarters of
//               the banks.  Both operands take their tokens in the same order, which is all a sum over tokens needs.
//     waves     a wave owns a 64 x 64 quarter as 2 x 2 accumulators of 32 x 32; per 16 tokens two A and two B operands feed four MFMAs.
//     epilogue  per 32 x 32 accumulator: H's tile is read (not when alpha == 0: NaN in unset memory does not survive), the two products
//               and the sum are rounded one by one, the block is stored, and for bi < bj the rounded beta S goes through LDS, turned, to
//               the same three steps on H's tile (bj, bi), so that both tiles are read and written along rows and EVERY entry of H is
//               scaled from its own old value.  A diagonal tile is computed whole: (i, j) and (j, i) sum the same exact
//               products in the same token order, the matrix comes out bit-symmetric.  Where n is an odd multiple of 64 the last panel is
//               half a tile: its upper columns are zeros in LDS and masked in the epilogue, the kernel shape is one.
//   Every entry is summed by one wave in one order fixed by `tokens` (stages of 32, the MFMA's own order within 16): no atomics, no split
//   of the token loop, nothing depends on the strides, the stream or the run.
//
//   Away from the intended design: ONE tile size for every n, where the host was to size the tile by n.  What a call moves at the
//   calibration shapes (2048 tokens, n = 4096: 128 MB of H against 34 Gflop) is bound by H's one read and one write, not by the
//   rounds of tiles, and a second shape would be a second summation order to pin; small n (fewer tiles than CUs) is left slow.
#ifndef QQQ_AMD_QQQ_HESSIAN_HIP_H_
#define QQQ_AMD_QQQ_HESSIAN_HIP_H_

#pragma clang fp contract(off)

static constexpr int HES_NT = 256;            // four waves
static constexpr int HES_TILE = 128;          // tile edge; a wave owns 64 x 64
static constexpr int HES_TS = 32;             // tokens of a stage: two MFMA steps
static constexpr int HES_LD = HES_TILE + 32;  // LDS row stride of a staged panel in halves (320 bytes)
static constexpr int HES_TLD = 33;            // row stride of a wave's 32 x 32 transpose buffer in floats

typedef _Float16 hes_h8 __attribute__((ext_vector_type(8)));
typedef short hes_s4 __attribute__((ext_vector_type(4)));
typedef short hes_s8 __attribute__((ext_vector_type(8)));
typedef float hes_f16 __attribute__((ext_vector_type(16)));
typedef unsigned int hes_u4 __attribute__((ext_vector_type(4)));

struct qqq_hessian_args {
  float* H;
  const _Float16* X;
  long long ldh, ldx;
  int tokens, n;
  int nb;      // panels of 128 columns: ceil(n / 128)
  int ntiles;  // nb (nb + 1) / 2
  float alpha, beta;
};

// one 32 x 16 MFMA operand from a staged panel: columns col0 ... col0 + 31, tokens tok0 ... tok0 + 15 (lanes 0 - 31 the tokens
// 0 - 7, lanes 32 - 63 the tokens 8 - 15, a lane's column is lane % 32).  ds_read_b64_tr_b16: per 16-lane group four rows x sixteen
// columns, lane 4 q + p gives the address of row q, columns 4 p ... 4 p + 3, and receives column (lane % 16), rows 0 - 3.
__device__ __forceinline__ hes_h8 hes_operand(const _Float16* panel, const int tok0, const int col0, const int lane) {
  const int g = lane >> 4, c = lane & 15;
  const _Float16* p = panel + (tok0 + 8 * (g >> 1) + (c >> 2)) * HES_LD + col0 + 16 * (g & 1) + 4 * (c & 3);
  const hes_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) hes_s4*)(p));
  const hes_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) hes_s4*)(p + 4 * HES_LD));
  const hes_s8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(hes_h8, v);
}

__global__ __launch_bounds__(HES_NT) void qqq_hessian_kernel(const qqq_hessian_args a) {
  __shared__ __attribute__((aligned(16))) _Float16 stage[2][2][HES_TS * HES_LD];  // [buffer][row panel, column panel]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 1, wc = w & 1;

  // workgroup b runs on XCD b % 8: every XCD takes one contiguous run of the column-by-column order of the triangle
  int bi, bj;
  {
    const int q = a.ntiles >> 3, rr = a.ntiles & 7;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    fac_tri((xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + idx, bi, bj);
  }
  const bool diag = bi == bj;
  const int np = diag ? 1 : 2;  // panels to stage

  // staging: thread -> (row r0 and r0 + 16 of the stage, 16-byte chunk ch of the panel's 128 columns)
  const int r0 = tid >> 4, ch = tid & 15;
  const int colA = bi * HES_TILE + 8 * ch, colB = bj * HES_TILE + 8 * ch;
  const bool liveA = colA < a.n, liveB = colB < a.n;  // (n is a multiple of 64: a chunk is inside or outside as a whole)
  hes_u4 regs[2][2];
  auto fetch = [&](const int t0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int t = t0 + r0 + 16 * h;
      const bool row = t < a.tokens;
      const _Float16* xr = a.X + (long long)(row ? t : 0) * a.ldx;
      regs[0][h] = row && liveA ? *reinterpret_cast<const hes_u4*>(xr + colA) : hes_u4{0u, 0u, 0u, 0u};
      if (!diag) regs[1][h] = row && liveB ? *reinterpret_cast<const hes_u4*>(xr + colB) : hes_u4{0u, 0u, 0u, 0u};
    }
  };
  auto park = [&](const int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
      for (int p = 0; p < np; ++p) *reinterpret_cast<hes_u4*>(&stage[buf][p][(r0 + 16 * h) * HES_LD + 8 * ch]) = regs[p][h];
  };

  hes_f16 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[u][v][r] = 0.f;

  const int stages = (a.tokens + HES_TS - 1) / HES_TS;
  fetch(0);
  park(0);
  __syncthreads();
  for (int s = 0; s < stages; ++s) {
    const int buf = s & 1;
    if (s + 1 < stages) fetch((s + 1) * HES_TS);
    const _Float16* pa = stage[buf][0];
    const _Float16* pb = stage[buf][diag ? 0 : 1];
#pragma unroll
    for (int k = 0; k < HES_TS; k += 16) {
      hes_h8 fa[2], fb[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        fa[u] = hes_operand(pa, k, 64 * wr + 32 * u, lane);
        fb[u] = hes_operand(pb, k, 64 * wc + 32 * u, lane);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[u], fb[v], acc[u][v], 0, 0, 0);
    }
    if (s + 1 < stages) park(buf ^ 1);
    __syncthreads();  // the next stage is in place, and nobody reads this one any more
  }

  // epilogue.  An accumulator holds, in register r of lane l, row 8 (r / 4) + 4 (l / 32) + r % 4 and column l % 32 of its block.
  // The staging buffers are free behind the loop's last barrier: every wave turns its blocks in 32 x 33 floats of its own.
  float* turn = reinterpret_cast<float*>(&stage[0][0][0]) + w * (32 * HES_TLD);
  const int lc = lane & 31, lh = lane >> 5;
  const bool read_h = a.alpha != 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int i0 = bi * HES_TILE + 64 * wr + 32 * u, j0 = bj * HES_TILE + 64 * wc + 32 * v;  // (a block is inside n or outside as a whole)
      const bool live = i0 < a.n && j0 < a.n;
      if (live) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = 8 * (r >> 2) + 4 * lh + (r & 3);
          float* hp = a.H + (long long)(i0 + i) * a.ldh + j0 + lc;
          const float scaled = a.beta * acc[u][v][r];
          const float kept = read_h ? a.alpha * *hp : 0.f;
          const float out = kept + scaled;
          *hp = out;
          if (!diag) turn[i * HES_TLD + lc] = scaled;
        }
      }
      if (!diag) {  // (uniform over the workgroup: the barriers are met by every wave)
        __syncthreads();
        if (live) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int j = 2 * r + lh;  // row j0 + j of the mirrored block takes column j of the block, along i
            float* hp = a.H + (long long)(j0 + j) * a.ldh + i0 + lc;
            const float kept = read_h ? a.alpha * *hp : 0.f;
            *hp = kept + turn[lc * HES_TLD + j];
          }
        }
        __syncthreads();
      }
    }
}

#endif  // QQQ_AMD_QQQ_HESSIAN_HIP_H_
