// qqq_factor.hip.h -- the kernels of qqq_upper_factor (qqq_amd/quant/include/qqq_amd_factor.h): U upper triangular with positive
// diagonal and U^T U = H^-1, by the direct route  H = R R^T (R upper: a Cholesky factorisation taken from the bottom-right corner
// upwards),  U = R^-1.  Part of the single translation unit qqq_quant.hip (floating-point contraction off).
//
// The matrix is cut into diagonal blocks of 128 columns taken from the END (rows / columns n - 128 ... n - 1 first); where n is an odd
// multiple of 64 the first block (rows 0 ... 63) is 64 wide.  Everything off the diagonal moves in 64 x 64 tiles.
//
//   qqq_factor_diag_kernel<BW>    one workgroup, the sequential spine.  The BW x BW diagonal block of the running matrix goes into LDS
//       (row stride BW + 1: a column walk touches every bank once).  Factorisation, column c from the last to the first, ONE barrier a
//       step: every thread reads the pivot a[c][c] and the column above it as the steps before left them, forms 1 / sqrt(pivot) and the
//       scaled column entries it needs itself (the same operations on the same bits in every thread, so nobody waits for a scaled
//       column), and subtracts r_ic * r_kc (product rounded, then subtracted) from its elements i <= k < c.  A wave owns rows (i % 4),
//       a lane the columns lane and lane + 64.  Behind the loop the columns are scaled once -- R.  Inversion in the same launch: thread c
//       owns column c of X = R^-1 in a second LDS matrix and back-substitutes R x = e_c in axpy form (k from c down: x_k *= 1 / r_kk,
//       x_i -= r_ik * x_k above it); the r_ik are wave-uniform LDS broadcasts, the x_i lane-consecutive, and no barrier is needed.  X is
//       written to U's diagonal block with zeros below the diagonal.  R_jj itself is never stored: only its inverse is used again.
//       The first pivot (in this order) that is <= 0 or NaN is kept in *info as 1 + its index; the arithmetic goes on (NaN), in bounds.
//   qqq_factor_gemm_kernel<BT, NEG>   one f32 MFMA tile template (v_mfma_f32_32x32x2_f32) for every product off the spine.  A workgroup
//       of four waves owns a 64 x 64 tile of C, a wave a 32 x 32 quarter: 16 accumulator registers that stay put over the whole k extent.
//       k runs in stages of 32: the 64 x 32 panels of A and B are fetched from global memory with 16-byte loads into registers WHILE the
//       MFMAs of the stage before run, then stored k-major into LDS (row stride 65), from where an MFMA operand is one conflict-free
//       4-byte read per lane.  BT: B is given [n][k] (C = A B^T) or [k][n] (C = A B).  NEG: C = Cin - A B (Cin may be absent: C = -A B).
//       Grid forms: rectangular (tile row, tile column), the upper triangle ti <= tk of a square of tiles as one linear index, and a k
//       range that starts at the tile row's own diagonal (A upper triangular).
//   qqq_factor_zero_kernel        zeros of the 64 x 64 tiles of U strictly below the diagonal (a linear index over them).
//
// The launch chain (qqq_quant.hip), per diagonal block J = [c0, c0 + bw) from the last to the first, src = H for the last block and the
// running copy W (workspace) afterwards -- H is never written and never copied as a whole:
//   diag   U_JJ = inv(chol_rev(src_JJ))
//   panel  U_iJ = src_iJ . U_JJ^T              rows above: R_iJ, parked in U's own upper triangle until the inverse pass replaces it
//   update W_ik = src_ik - U_iJ . U_kJ^T       upper tiles i <= k < J only
// then per block J ascending:
//   T   = U_{0:c0, J} . U_JJ                   (R_{0:c0, J} . U_JJ, into the workspace's n x 128 strip)
//   U_{0:c0, J} = - U_{0:c0, 0:c0} . T         k from the tile row's diagonal on
// Every tile is summed in one fixed order by one workgroup; no atomics.
#ifndef QQQ_AMD_QQQ_FACTOR_HIP_H_
#define QQQ_AMD_QQQ_FACTOR_HIP_H_

#pragma clang fp contract(off)

static constexpr int FAC_NT = 256;    // threads of every workgroup here
static constexpr int FAC_TILE = 64;   // tile edge of the GEMM template
static constexpr int FAC_KT = 32;     // k extent of a stage
static constexpr int FAC_LDT = FAC_TILE + 1;
static constexpr int FAC_BLOCK = 128; // widest diagonal block

typedef float fac_f4 __attribute__((ext_vector_type(4)));
typedef float fac_f16 __attribute__((ext_vector_type(16)));

// p = tk (tk + 1) / 2 + ti with 0 <= ti <= tk: the upper triangle of a square of tiles, column by column
__device__ __forceinline__ void fac_tri(const int p, int& ti, int& tk) {
  int k = (int)((sqrtf(8.f * (float)p + 1.f) - 1.f) * 0.5f);
  while (k > 0 && k * (k + 1) / 2 > p) --k;
  while ((k + 1) * (k + 2) / 2 <= p) ++k;
  tk = k;
  ti = p - k * (k + 1) / 2;
}

struct qqq_factor_diag_args {
  const float* src;  // the diagonal block of the running matrix (upper triangle read)
  float* U;          // the diagonal block of U
  int* info;
  long long lds, ldu;
  int base;          // index of the block's first column
  int first;         // 1: the chain's first launch writes *info unconditionally
};

template <int BW>
__global__ __launch_bounds__(FAC_NT) void qqq_factor_diag_kernel(const qqq_factor_diag_args a) {
  constexpr int LD = BW + 1;
  __shared__ float a_s[BW * LD];
  __shared__ float x_s[BW * LD];
  __shared__ float rinv_s[BW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int idx = tid; idx < BW * BW; idx += FAC_NT) {
    const int i = idx / BW, k = idx % BW;
    a_s[i * LD + k] = i <= k ? a.src[(long long)i * a.lds + k] : 0.f;
    x_s[i * LD + k] = i == k ? 1.f : 0.f;
  }
  int fail = 0;
  for (int c = BW - 1; c >= 0; --c) {
    __syncthreads();
    const float piv = a_s[c * LD + c];
    if (!(piv > 0.f) && fail == 0) fail = a.base + c + 1;
    const float rinv = 1.f / sqrtf(piv);
    float rk[BW / 64];
#pragma unroll
    for (int h = 0; h < BW / 64; ++h) {
      const int k = lane + 64 * h;
      rk[h] = k < c ? a_s[k * LD + c] * rinv : 0.f;
    }
    for (int i = wave; i < c; i += 4) {
      const float ri = a_s[i * LD + c] * rinv;
#pragma unroll
      for (int h = 0; h < BW / 64; ++h) {
        const int k = lane + 64 * h;
        if (k >= i && k < c) {
          const float prod = ri * rk[h];
          a_s[i * LD + k] = a_s[i * LD + k] - prod;
        }
      }
    }
  }
  __syncthreads();
  if (tid < BW) rinv_s[tid] = 1.f / sqrtf(a_s[tid * LD + tid]);
  __syncthreads();
  // R above the diagonal: every column scaled once (the diagonal is only used through rinv_s)
  for (int idx = tid; idx < BW * BW; idx += FAC_NT) {
    const int i = idx / BW, k = idx % BW;
    if (i < k) a_s[i * LD + k] = a_s[i * LD + k] * rinv_s[k];
  }
  __syncthreads();
  if (tid < BW) {
    const int c = tid;
    const int top = (wave + 1) * 64 < BW ? (wave + 1) * 64 - 1 : BW - 1;  // the wave's last column
    for (int k = top; k >= 0; --k) {
      if (k <= c) {
        const float xk = x_s[k * LD + c] * rinv_s[k];
        x_s[k * LD + c] = xk;
#pragma unroll 4
        for (int i = 0; i < k; ++i) {
          const float prod = a_s[i * LD + k] * xk;
          x_s[i * LD + c] = x_s[i * LD + c] - prod;
        }
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < BW * BW; idx += FAC_NT) {
    const int i = idx / BW, k = idx % BW;
    a.U[(long long)i * a.ldu + k] = i <= k ? x_s[i * LD + k] : 0.f;
  }
  if (tid == 0) {
    if (a.first)
      *a.info = fail;
    else if (fail != 0 && *a.info == 0)
      *a.info = fail;
  }
}

struct qqq_factor_gemm_args {
  const float* A;    // [rows][k], row stride lda; tile row ti starts at row 64 ti
  const float* B;    // BT: [n][k], tile column tj starts at row 64 tj.  else [k][n], tile column tj starts at column 64 tj
  const float* Cin;  // NEG only: what the product is subtracted from, or NULL
  float* C;
  long long lda, ldb, ldcin, ldc;
  int K;         // k extent, a multiple of 64
  int tri_grid;  // 1: blockIdx.x walks the upper triangle ti <= tj of a square of tiles
  int tri_k;     // 1: k starts at 64 ti
};

template <bool BT, bool NEG>
__global__ __launch_bounds__(FAC_NT) void qqq_factor_gemm_kernel(const qqq_factor_gemm_args a) {
  __shared__ float as_s[FAC_KT * FAC_LDT];
  __shared__ float bs_s[FAC_KT * FAC_LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  int ti, tj;
  if (a.tri_grid) {
    fac_tri((int)blockIdx.x, ti, tj);
  } else {
    ti = blockIdx.x;
    tj = blockIdx.y;
  }
  const int kb = a.tri_k ? FAC_TILE * ti : 0;
  // a panel in [row][k] form: eight threads take the 128 bytes of a row's stage, rows r and r + 32
  const int kq = tid & 7, r = tid >> 3;
  // B in [k][n] form: sixteen threads take the 256 bytes of a k row, rows kr and kr + 16
  const int nq = tid & 15, kr = tid >> 4;
  const float* Ap = a.A + ((long long)FAC_TILE * ti + r) * a.lda + 4 * kq;
  const float* Bp = BT ? a.B + ((long long)FAC_TILE * tj + r) * a.ldb + 4 * kq : a.B + (long long)kr * a.ldb + FAC_TILE * tj + 4 * nq;
  const long long a_half = 32 * a.lda, b_half = BT ? 32 * a.ldb : 16 * a.ldb;

  fac_f4 ra[2], rb[2];
  auto fetch = [&](const int k0) {
    ra[0] = *reinterpret_cast<const fac_f4*>(Ap + k0);
    ra[1] = *reinterpret_cast<const fac_f4*>(Ap + a_half + k0);
    const float* bp = BT ? Bp + k0 : Bp + (long long)k0 * a.ldb;
    rb[0] = *reinterpret_cast<const fac_f4*>(bp);
    rb[1] = *reinterpret_cast<const fac_f4*>(bp + b_half);
  };

  fac_f16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;

  fetch(kb);
  for (int k0 = kb; k0 < a.K; k0 += FAC_KT) {
    __syncthreads();  // the stage before is read
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        as_s[(4 * kq + e) * FAC_LDT + r + 32 * p] = ra[p][e];
        if (BT)
          bs_s[(4 * kq + e) * FAC_LDT + r + 32 * p] = rb[p][e];
        else
          bs_s[(kr + 16 * p) * FAC_LDT + 4 * nq + e] = rb[p][e];
      }
    __syncthreads();
    if (k0 + FAC_KT < a.K) fetch(k0 + FAC_KT);  // in flight under this stage's MFMAs
    const float* ap = as_s + (lane >> 5) * FAC_LDT + 32 * wm + (lane & 31);
    const float* bp = bs_s + (lane >> 5) * FAC_LDT + 32 * wn + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < FAC_KT; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk * FAC_LDT], bp[kk * FAC_LDT], acc, 0, 0, 0);
  }

  // D[i][j] of a 32 x 32 MFMA: j = lane % 32, i = 8 (v / 4) + 4 (lane / 32) + v % 4
  const long long col = (long long)FAC_TILE * tj + 32 * wn + (lane & 31);
  const long long row0 = (long long)FAC_TILE * ti + 32 * wm + 4 * (lane >> 5);
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const long long row = row0 + 8 * (v / 4) + v % 4;
    float out = acc[v];
    if (NEG) out = a.Cin ? a.Cin[row * a.ldcin + col] - out : -out;
    a.C[row * a.ldc + col] = out;
  }
}

struct qqq_factor_zero_args {
  float* U;
  long long ldu;
};

// blockIdx.x = p over the pairs tk < ti of 64-tiles (the strict lower triangle, by fac_tri on a square one smaller)
__global__ __launch_bounds__(FAC_NT) void qqq_factor_zero_kernel(const qqq_factor_zero_args a) {
  int lo, hi;
  fac_tri((int)blockIdx.x, lo, hi);  // lo <= hi: the tile at row hi + 1, column lo
  const int tid = threadIdx.x, q = tid & 15, r = tid >> 4;
  float* p = a.U + ((long long)FAC_TILE * (hi + 1) + r) * a.ldu + FAC_TILE * lo + 4 * q;
  const fac_f4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s) *reinterpret_cast<fac_f4*>(p + 16 * s * a.ldu) = z;
}

#endif  // QQQ_AMD_QQQ_FACTOR_HIP_H_
